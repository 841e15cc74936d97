"""mfh_newmark on the device against the reference recurrence of tests/dynamics_util.py (the Newmark scheme on the oracle's pencil with sparse
direct solves) and against closed forms, on the small meshes of tests/modes_util.py and on its mid mesh. rtol = 1e-12 unless a test says otherwise.
Bars, with the reference measurements they come from (the recurrence with its solves replaced by scipy CG deviates from itself, over 100 steps
at dt = T_1 / 20, by at most 108 rtol per snapshot in rel-L2 and 11 rtol of the energies' maximum; the device gets about 9 x that for its other
preconditioner and summation order):
  snapshots    every snapshot rel-L2 <= 1e3 rtol against the recurrence
  energies     <= 1e2 rtol of the maximum of each column
  probes       equal to the snapshot entries bit for bit
  dispersion   against phi cos(n theta): <= 1e3 rtol + the direct recurrence's own defect (computed here)
  invariants   |E_n / E_0 - 1| <= 1e2 rtol undamped and unloaded; E - f.u constant to 1e2 rtol max E under a constant load; damped: E never increases
  static limit one step of dt = 1e4 T_1 from rest: the mfh_solve solution to 4 / (omega_1 dt)^2 + 1e3 rtol in the oracle's M-norm
  kernels      worst-case rounding bounds (each test states its own)
Every run is made once (functools.lru_cache) and shared by the tests that look at it."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import meshfem_amd as M
from meshfem_amd import _lib

import dynamics_util as D
import modes_util as U

pytestmark = pytest.mark.gpu

RTOL = 1e-12
EPS = U.EPS
PRECONDS = {"jacobi": M.PRECOND_BLOCK_JACOBI, "two-level": M.PRECOND_TWO_LEVEL, "multigrid": M.PRECOND_MULTIGRID}


def _is3d(key):
    return key == U.MID or key[0] == 3


def _name(key):
    return key if isinstance(key, str) else "%dD-P%d" % key


def _context(key, precond="jacobi", options=(), clamped=True):
    V, T, deg, _ = U.mesh_arrays(key)
    c = M.Context(0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    c.set_preconditioner(PRECONDS[precond])
    if clamped:
        c.fix_variables(U.clamp_vars(key))
    return c


def _probe_vars(key, clamped=True):
    free = D.free_of(key, clamped)
    return np.array([free[0], free[len(free) // 2], free[-1], free[0]], dtype=np.int64)


def _run_case(c, key, case, n_steps=100, clamped=True, **kw):
    i = D.case_inputs(key, case, n_steps, clamped)
    args = dict(u0=i["u0"], v0=i["v0"], f=i["f"], amplitude=i["amplitude"], density=i["density"], damping=i["damping"], rtol=RTOL, maxit=20000,
                probes=_probe_vars(key, clamped), snapshot_stride=1, energies=True)
    args.update(kw)
    return c.newmark(i["dt"], n_steps, **args)


@functools.lru_cache(maxsize=None)
def _device_run(key, case, precond, n_steps=100, clamped=True):
    c = _context(key, precond, clamped=clamped)
    assert np.array_equal(c.node_positions(), U.fem_mesh(key).node_pos)          # the oracle's node numbering is the library's own
    r = _run_case(c, key, case, n_steps, clamped)
    c.close()
    return r


def _check_against_reference(r, key, case, n_steps=100, clamped=True):
    Uref, Vref, Aref, Eref = D.reference_run(key, case, n_steps, clamped)
    err = D.rel_l2_rows(r["snapshots"], Uref)
    eerr = (np.abs(r["energies"] - Eref).max(axis=0) / np.abs(Eref).max(axis=0)).max()
    info = r["info"]
    print("%s %s: snapshots %.3e (bar %.1e), energies %.3e (bar %.1e); %d + %d iterations, worst step %d, note '%s'" %
          (_name(key), case, err, 1e3 * RTOL, eerr, 1e2 * RTOL, info["iterationsInit"], info["iterationsTotal"], info["iterationsMax"], info["note"]))
    assert info["stepsDone"] == n_steps
    assert err <= 1e3 * RTOL
    assert eerr <= 1e2 * RTOL
    pv = _probe_vars(key, clamped)
    assert np.array_equal(r["probes"], r["snapshots"][:, pv])
    assert np.array_equal(r["u"], r["snapshots"][-1])
    assert D.rel_l2_rows(r["v"][None, :], Vref[-1:]) <= 1e3 * RTOL
    fixed = np.setdiff1d(np.arange(Uref.shape[1]), D.free_of(key, clamped))
    assert np.all(r["snapshots"][:, fixed] == 0.0) and np.all(r["v"][fixed] == 0.0) and np.all(r["a"][fixed] == 0.0)


REFERENCE_CASES = [(k, p) for k in U.SMALL for p in ("jacobi", "two-level", "multigrid")]


@pytest.mark.parametrize("case", ["undamped", "damped"])
@pytest.mark.parametrize("key,precond", REFERENCE_CASES, ids=_name)
def test_against_the_reference_recurrence(key, precond, case):
    """100 steps at dt = T_1 / 20, random amplitude table, non-zero u0 and v0, a snapshot at every step, every preconditioner; undamped and
    Rayleigh-damped with aR = 0.1 omega_1, bR = 0.02 / omega_1."""
    r = _device_run(key, case, precond)
    _check_against_reference(r, key, case)
    want, used = PRECONDS[precond], r["info"]["precondUsed"]
    print("%s %s: asked for %s, precondUsed %d" % (_name(key), case, precond, used))
    if key == (3, 2):
        assert used == want                                   # both hierarchies build on the quadratic tets: the two-level and the V-cycle path ran
    elif used != want:
        assert r["info"]["note"]                              # the hierarchy does not apply to this mesh: the note says what ran instead
        assert ("block-Jacobi" in r["info"]["note"]) == (used == M.PRECOND_BLOCK_JACOBI)


@pytest.mark.parametrize("j", [0, 2])
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_dispersion(key, j):
    """Started from mode j of the clamped pencil at rest, no load: u_n = phi cos(n theta) -- independent of the oracle's recurrence, whose own defect
    against the closed form is added to the bar."""
    _, closed, defect = D.dispersion_reference(key, j)
    phi, _ = D.mode_shape(key, j)
    c = _context(key, "multigrid")
    dt = 2.0 * np.pi / D.omega1(key) / 20.0
    r = c.newmark(dt, 60, u0=phi, density=D.DENSITY, rtol=RTOL, maxit=20000, snapshot_stride=1)
    c.close()
    err = np.linalg.norm(r["snapshots"] - closed, axis=1).max() / np.linalg.norm(phi)
    print("%s mode %d: error %.3e, the direct recurrence's defect %.3e" % (_name(key), j, err, defect))
    assert err <= 1e3 * RTOL + defect


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_invariants(key):
    i = D.case_inputs(key, "undamped")
    c = _context(key, "multigrid")
    common = dict(u0=i["u0"], v0=i["v0"], density=i["density"], rtol=RTOL, maxit=20000, energies=True)
    E = c.newmark(i["dt"], 100, **common)["energies"]
    tot = E[:, 0] + E[:, 1]
    drift = np.abs(tot / tot[0] - 1).max()
    E = c.newmark(i["dt"], 100, f=i["f"], **common)["energies"]
    bal = E[:, 0] + E[:, 1] - E[:, 2]
    wdrift = np.abs(bal - bal[0]).max() / (E[:, 0] + E[:, 1]).max()
    damped = D.case_inputs(key, "damped")["damping"]
    E = c.newmark(i["dt"], 100, damping=damped, **common)["energies"]
    c.close()
    dtot = E[:, 0] + E[:, 1]
    rise = np.diff(dtot).max() / dtot[0]
    print("%s: energy drift %.3e, work-balance drift %.3e (bar %.1e), largest change of E under damping %.3e of E_0" % (_name(key), drift, wdrift, 1e2 * RTOL, rise))
    assert drift <= 1e2 * RTOL
    assert wdrift <= 1e2 * RTOL
    assert np.diff(dtot).max() <= 0 and dtot[-1] < 0.9 * dtot[0]


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_static_limit(key):
    """From rest with the load switched on after step 0 (g = 0, 1), one step of dt = 1e4 T_1: (K + 4 M / dt^2) u_1 = f, whose distance from
    K^-1 f is at most 4 / (omega_1 dt)^2 per mode in the M-norm."""
    i = D.case_inputs(key, "undamped")
    w1 = D.omega1(key)
    dt = 1e4 * 2.0 * np.pi / w1
    c = _context(key, "multigrid")
    r = c.newmark(dt, 1, f=i["f"], amplitude=[0.0, 1.0], density=i["density"], rtol=RTOL, maxit=20000)
    us = c.solve(i["f"], rtol=RTOL)
    c.close()
    _, Mm = U.pencil(key)
    d = r["u"] - us
    err = np.sqrt((d @ (Mm @ d)) / (us @ (Mm @ us)))
    bar = 4.0 / (w1 * dt) ** 2 + 1e3 * RTOL
    print("%s: ||u_1 - u_static||_M / ||u_static||_M = %.3e (bar %.3e), %d iterations" % (_name(key), err, bar, r["info"]["iterationsTotal"]))
    assert r["info"]["iterationsInit"] == 0          # a zero right-hand side: a0 = 0 without an iteration
    assert err <= bar


@pytest.mark.parametrize("deterministic", [1, 0], ids=["deterministic", "default"])
def test_chaining(deterministic):
    """50 + 50 steps through (u, v, a) equal 100 steps: bit for bit under option deterministic (where two identical calls are bit-identical too),
    within the snapshot bar otherwise."""
    key, case = (3, 2), "damped"
    i = D.case_inputs(key, case)
    c = _context(key, "multigrid", (("deterministic", deterministic),))
    whole = _run_case(c, key, case)
    first = _run_case(c, key, case, n_steps=50, amplitude=i["amplitude"][:51])
    second = _run_case(c, key, case, n_steps=50, amplitude=i["amplitude"][50:], u0=first["u"], v0=first["v"], a0=first["a"])
    assert second["info"]["iterationsInit"] == 0
    snaps = np.vstack([first["snapshots"], second["snapshots"][1:]])
    assert np.array_equal(second["snapshots"][0], first["snapshots"][-1])
    if deterministic:
        again = _run_case(c, key, case)
        for k in ("u", "v", "a", "snapshots", "probes", "energies"):
            assert np.array_equal(again[k], whole[k]), k
        assert np.array_equal(snaps, whole["snapshots"])
        for k in ("u", "v", "a"):
            assert np.array_equal(second[k], whole[k]), k
        assert np.array_equal(np.vstack([first["energies"], second["energies"][1:]]), whole["energies"])
    else:
        err = D.rel_l2_rows(snaps, whole["snapshots"])
        print("chained against whole: %.3e" % err)
        assert err <= 1e3 * RTOL
    c.close()


@pytest.mark.parametrize("precond", ["jacobi", "multigrid"])
@pytest.mark.parametrize("key", [(2, 2), (3, 1)], ids=_name)
def test_no_fixed_variables(key, precond):
    """The free body: K is singular, A = cK K + cM M is not. Against the reference on the unclamped pencil; the note names block-Jacobi."""
    r = _device_run(key, "damped", precond, 100, False)
    _check_against_reference(r, key, "damped", 100, False)
    assert "block-Jacobi" in r["info"]["note"] and r["info"]["precondUsed"] == M.PRECOND_BLOCK_JACOBI


def test_mid_mesh():
    """8 x 7 x 6 quadratic tets (37 905 unknowns: kernels of many workgroups), multigrid, 20 steps against the splu recurrence."""
    r = _device_run(U.MID, "undamped", "multigrid", 20)
    _check_against_reference(r, U.MID, "undamped", 20)
    assert r["info"]["precondUsed"] == M.PRECOND_MULTIGRID


def test_simulator_layer_under_a_periodic_dof_map():
    """Simulator.transient on the periodic bar (fewer DoFs than nodes, no Dirichlet condition: the free body): nodal fields in, nodal fields out, the
    probes remapped to the DoFs -- the same bits as Context.newmark on the DoF vectors (option deterministic 1)."""
    from meshfem_amd.linear_elasticity import Simulator
    V, T, deg, _ = U.mesh_arrays(U.BAR)
    sim = Simulator(T, V, deg)
    sim.ctx.set_option("deterministic", 1)
    sim.setIsotropicMaterial(U.E_MOD, U.NU)
    sim.applyPeriodicConditions()
    ctx = sim.ctx
    assert ctx.n_dof < ctx.n_node
    dof, _ = ctx.get_dof_map()
    rng = np.random.default_rng(2)
    ud, vd = rng.standard_normal((2, ctx.n_dof, 3))
    shared = int(np.nonzero(dof != np.arange(ctx.n_node))[0][-1])          # a node that is not the first of its DoF
    probes = [(shared, 1), (0, 2), (ctx.n_node // 2, 0)]
    args = dict(density=1.7, damping=(0.1, 0.01), snapshot_stride=1, energies=True, rtol=1e-10, maxit=5000)
    res = sim.transient(0.5, 5, u0=ud[dof], v0=vd[dof], probes=probes, **args)
    pv = [int(dof[n_]) * 3 + a for n_, a in probes]
    direct = ctx.newmark(0.5, 5, u0=ud.reshape(-1), v0=vd.reshape(-1), probes=pv, **args)
    assert sim.transient_info["stepsDone"] == 5 and "block-Jacobi" in sim.transient_info["note"]
    assert res["u"].shape == (ctx.n_node, 3) and res["snapshots"].shape == (6, ctx.n_node, 3)
    for k in ("u", "v", "a"):
        assert np.array_equal(res[k], direct[k].reshape(ctx.n_dof, 3)[dof]), k
    assert np.array_equal(res["snapshots"], direct["snapshots"].reshape(6, ctx.n_dof, 3)[:, dof, :])
    assert np.array_equal(res["snapshots"][0], ud[dof])
    assert np.array_equal(res["probes"], direct["probes"]) and np.array_equal(res["energies"], direct["energies"])
    for j, (n_, a) in enumerate(probes):
        assert np.array_equal(res["probes"][:, j], res["snapshots"][:, n_, a])
    ctx.close()


def _probe(c):
    """What test_nothing_existing_moves compares: a solve, K x, the exported triplets, the modes."""
    n = c.bs * c.n_dof
    rng = np.random.default_rng(5)
    f, x = rng.standard_normal(n), rng.standard_normal(n)
    u = c.solve(f, rtol=1e-9)
    kx = c.apply_K(x)
    trip = c.export_upper_triplets()
    lam, X, _ = c.modes(3, rtol=1e-6)
    return [u, kx, lam, X] + list(trip)


@pytest.mark.parametrize("storage", [-1, 0], ids=["default-storage", "both-triangles"])
def test_nothing_existing_moves(storage):
    """A context that has run mfh_newmark solves, applies K, exports and finds modes like a fresh one, bit for bit -- also the default quadratic
    context, whose pattern the call widened to both triangles for its own duration (option deterministic 1 on both, as in test_gpu_modes.py)."""
    key = (3, 2)
    opts = (("deterministic", 1), ("matrix_storage", storage))
    a = _context(key, "multigrid", opts)
    r = _run_case(a, key, "damped", n_steps=5, amplitude=D.case_inputs(key, "damped")["amplitude"][:6])
    assert r["info"]["stepsDone"] == 5
    assert ("both triangles" in r["info"]["note"]) == (storage == -1)
    got = _probe(a)
    b = _context(key, "multigrid", opts)
    want = _probe(b)
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)
    a.close(); b.close()


def test_maxit_one():
    key = (3, 2)
    i = D.case_inputs(key, "undamped")
    c = _context(key, "jacobi")
    for a0 in (None, np.zeros_like(i["u0"])):           # the solve for a0 fails / the first step fails
        with pytest.raises(M.MeshFEMHipError) as ei:
            c.newmark(i["dt"], 3, u0=i["u0"], v0=i["v0"], a0=a0, f=i["f"], density=i["density"], rtol=RTOL, maxit=1)
        assert ei.value.code == _lib.ERR_NOT_CONVERGED
        r = c.last_newmark
        assert r["info"]["stepsDone"] == 0
        assert np.array_equal(r["u"], i["u0"]) and np.array_equal(r["v"], i["v0"]) and np.all(r["a"] == 0.0)
    n = c.bs * c.n_dof
    u = c.solve(np.ones(n), rtol=1e-8)
    assert c.last_info["converged"] == 1 and np.all(np.isfinite(u))
    r = c.newmark(i["dt"], 2, u0=i["u0"], v0=i["v0"], f=i["f"], density=i["density"], rtol=1e-8)
    assert r["info"]["stepsDone"] == 2
    c.close()


@pytest.mark.parametrize("precond", ["jacobi", "multigrid"])
def test_loop_kernels_past_their_grid_cap(precond):
    """The PCG's vector kernels and k_spmv_kron_acc run up to 2 048 workgroups, more than any test mesh fills. Option dyn_grid_cap 1 leaves them one
    workgroup, whose lanes then loop over the rows (and whose 256 lanes walk every row chunk): the same bars against the recurrence, and the pencil
    product against the default grid to the rounding of another summation order of x . y (y itself: the same bits -- under option deterministic,
    because each call assembles M anew on this upper-storage context and the default assembly adds in arrival order)."""
    key, case = (3, 2), "damped"
    c = _context(key, precond, (("dyn_grid_cap", 1), ("deterministic", 1)))
    r = _run_case(c, key, case, n_steps=20)
    _check_against_reference(r, key, case, 20)
    x = np.random.default_rng(9).standard_normal(c.bs * c.n_dof)
    y1, d1 = c.debug_pencil_apply(1.3, 47.0, x)
    c.set_option("dyn_grid_cap", 2048)
    y2, d2 = c.debug_pencil_apply(1.3, 47.0, x)
    c.close()
    assert np.array_equal(y1, y2)
    assert abs(d1 - d2) <= (len(x) + 4) * EPS * (np.abs(x) @ np.abs(y1))


# ---- the step kernels through their hooks, past their grid cap: they run 256 workgroups of 256 lanes at most (n = 100 003 makes the lanes loop)
SIZES = [1, 63, 64, 65, 1000, 100003]


@functools.lru_cache(maxsize=None)
def _hook_context():
    V, T, deg, _ = U.mesh_arrays((2, 1))
    c = M.Context(0)
    c.mesh_build(T, V, deg)
    return c


@pytest.mark.parametrize("n", SIZES)
def test_step_kernels_against_numpy(n):
    """Every output is a handful of fused multiply-adds of the inputs: |error| <= 4 eps x the sum of the moduli of its terms; b . b is a sum of n
    squares in another order: (n + 4) eps b . b."""
    c = _hook_context()
    rng = np.random.default_rng(n)
    dt, beta, gamma, rho, aR, bR = 0.37, 0.3, 0.6, 1.7, 0.21, 0.013
    u, v, a = rng.standard_normal((3, n))
    mask = (rng.random(n) < 0.2).astype(np.uint8) if n > 1 else np.zeros(1, dtype=np.uint8)
    free = mask == 0
    ut, vt, xm, xk = c.debug_newmark_predict(dt, beta, gamma, rho, (aR, bR), u, v, a, mask)
    cua, cva, cw = dt * dt * (0.5 - beta), dt * (1 - gamma), gamma / (beta * dt)
    rut, rvt = (u + dt * v + cua * a) * free, (v + cva * a) * free
    but, bvt = (np.abs(u) + np.abs(dt * v) + np.abs(cua * a)) * free, (np.abs(v) + np.abs(cva * a)) * free
    w, bw = cw * rut - rvt, np.abs(cw) * but + bvt
    cmu = rho / (beta * dt * dt)
    assert np.all(np.abs(ut - rut) <= 4 * EPS * but) and np.all(np.abs(vt - rvt) <= 4 * EPS * bvt)
    assert np.all(np.abs(xm - (cmu * rut + rho * aR * w)) <= 8 * EPS * (cmu * but + rho * aR * bw))
    assert np.all(np.abs(xk - bR * w) <= 8 * EPS * bR * bw)
    assert np.all(ut[~free] == 0) and np.all(vt[~free] == 0)
    # no mask, no K vector
    ut2, vt2, xm2, xk2 = c.debug_newmark_predict(dt, beta, gamma, rho, (aR, bR), u, v, a, None, want_xk=False)
    assert xk2 is None and np.array_equal(ut2[free], ut[free]) and np.array_equal(xm2[free], xm[free])
    # right-hand side
    f, y, g = rng.standard_normal(n), rng.standard_normal(n), -0.83
    b, bb = c.debug_newmark_rhs(g, f, y, mask)
    rb = (g * f + y) * free
    assert np.all(np.abs(b - rb) <= 4 * EPS * (np.abs(g * f) + np.abs(y))) and np.all(b[~free] == 0)
    assert abs(bb - b @ b) <= (n + 4) * EPS * (b @ b)
    b2, bb2 = c.debug_newmark_rhs(g, None, y, None)
    assert np.array_equal(b2, y) and abs(bb2 - y @ y) <= (n + 4) * EPS * (y @ y)
    # corrector
    x = rng.standard_normal(n)
    pv = rng.integers(0, n, size=7)
    un, vn, an, pout, snap = c.debug_newmark_correct(dt, beta, gamma, x, ut, vt, pv)
    ca = 1.0 / (beta * dt * dt)
    ra = ca * (x - ut)
    assert np.array_equal(un, x) and np.array_equal(snap, x) and np.array_equal(pout, x[pv])
    assert np.all(np.abs(an - ra) <= 4 * EPS * ca * (np.abs(x) + np.abs(ut)))
    assert np.all(np.abs(vn - (vt + gamma * dt * ra)) <= 8 * EPS * (np.abs(vt) + gamma * dt * ca * (np.abs(x) + np.abs(ut))))


@functools.lru_cache(maxsize=None)
def _device_pencil(key):
    """(K, M) as the device holds them (the exports of a second context under each operator)."""
    V, T, deg, _ = U.mesh_arrays(key)
    c = M.Context(0)
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    n = c.bs * c.n_dof
    out = []
    for op in (M.OP_ELASTICITY, M.OP_MASS_VECTOR):
        c.set_operator(op)
        c.assemble()
        i, j, v = c.export_upper_triplets()
        U_ = sp.coo_matrix((v, (i.astype(np.int64), j.astype(np.int64))), shape=(n, n)).tocsr()
        out.append(sp.csr_matrix(U_ + sp.triu(U_, 1).T))
    c.close()
    return tuple(out)


@pytest.mark.parametrize("matrix_free", [1, 0], ids=["matrix-free", "assembled"])
@pytest.mark.parametrize("key", [(2, 1), (3, 2), U.MID], ids=_name)
def test_pencil_product_against_scipy(key, matrix_free):
    """y = cK K x + cM M x, masked and unmasked, cK = 0 included. A row is a sum of L <= (row length) products per operator, the K entries
    themselves sums of some tens of element terms: |error| <= 4 L eps (|cK| |K| + |cM| |M|) |x| componentwise; x . y likewise from |x| . |y| terms."""
    K, Mm = _device_pencil(key)
    n = K.shape[0]
    L = int(np.diff(K.indptr).max())
    c = _context(key, "jacobi", (("matrix_free", matrix_free),) + ((("matrix_storage", 0),) if not matrix_free else ()))
    rng = np.random.default_rng(3)
    x = rng.standard_normal(n)
    fixed = U.clamp_vars(key)
    for cK, cM in ((1.3, 47.0), (0.0, 2.5), (1.0, 0.0)):
        for masked in (True, False):
            xin = x.copy()
            if masked:
                xin[fixed] = 0.0
            y, dot = c.debug_pencil_apply(cK, cM, xin, masked)
            ref = cK * (K @ xin) + cM * (Mm @ xin)
            bound = 4 * L * EPS * (abs(cK) * (abs(K) @ np.abs(xin)) + abs(cM) * (abs(Mm) @ np.abs(xin)))
            if masked:
                ref[fixed] = 0.0
                assert np.all(y[fixed] == 0.0)
            worst = (np.abs(y - ref) / np.where(bound > 0, bound, 1.0)).max()
            print("%s cK %.1f cM %.1f masked %d: worst error / bound %.3e" % (_name(key), cK, cM, masked, worst))
            assert np.all(np.abs(y - ref) <= bound)
            assert abs(dot - xin @ y) <= (n + 4) * EPS * (np.abs(xin) @ np.abs(y))
    c.close()
