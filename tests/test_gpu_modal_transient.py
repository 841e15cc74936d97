"""Modal transient response on the device (mfh_modal_transient) against the references of tests/modal_transient_util.py on scipy's (lam, X) of
tests/modal_util.py: the long-double twin of the recurrence, the dense exact solution on the 56-unknown mesh, Context.solve / Context.newmark on
the same context where the statement is about them. The bars come from the twin's own float64 defect (x 10), the rounding bound of the expansion
(modal_util.expand_bound) and the static solve's rtol, never from the device's output; tests/test_modal_transient_reference.py shows on the CPU
that the twin is the right reference."""
import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import _lib

import harmonic_util as H
import modal_transient_util as T
import modal_util as MU
import modes_util as U

pytestmark = pytest.mark.gpu

EPS = T.EPS
RTOL = MU.RTOL_STATIC
MAXIT = 20000
N_STEPS = 200
PRECONDS = {"jacobi": M.PRECOND_BLOCK_JACOBI, "two-level": M.PRECOND_TWO_LEVEL, "multigrid": M.PRECOND_MULTIGRID}


def _name(key):
    return key if isinstance(key, str) else "%dD-P%d" % key


def _context(key, precond="multigrid", options=(), clamped=True):
    V, Tt, deg, _ = U.mesh_arrays(key)
    c = M.Context(0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(Tt, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    c.set_preconditioner(PRECONDS[precond])
    if clamped:
        c.fix_variables(U.clamp_vars(key))
    return c


def _basis(key, m):
    lam, X = MU.clamped_basis(key)
    return lam[:m], X[:m]


def _code(call):
    with pytest.raises(M.MeshFEMHipError) as ei:
        call()
    return ei.value.code


def _run_args(key, case, m):
    aR, bR, zeta = T.damping_case(key, case, m)
    return dict(damping=(aR, bR), modal_damping=zeta, rtol=RTOL, maxit=MAXIT), (aR, bR, zeta)


def _mode_bars(X, f, g, defect, QL, VL, n_free):
    """Per mode, the bar on |q - q_twin| and |q' - q'_twin|: (10 defect + the relative rounding bound of the device's own g_j = phi_j^T f, a Gram sum over
    n_free rows: (n_free + 8) eps |phi_j|^T |f| / |g_j|) x max_n |q_j| -- q is linear in g, and the twin is run on numpy's g."""
    gb = (n_free + 8) * EPS * (np.abs(X) @ np.abs(f)) / np.where(g != 0, np.abs(g), 1.0)
    return (10 * defect + gb) * np.abs(QL).max(axis=0).astype(np.float64), (10 * defect + gb) * np.abs(VL).max(axis=0).astype(np.float64)


def _load_case(key):
    """dt at 12 points per period of mode 24 (or the last one), a random amplitude table."""
    lam = MU.clamped_basis(key)[0]
    dt = 2.0 * np.pi / np.sqrt(lam[min(23, len(lam) - 1)]) / 12.0
    return dt, np.random.default_rng(23).standard_normal(N_STEPS + 1)


# ---------------------------------------------------------------- against the twin on the same modes
@pytest.mark.parametrize("case", T.DAMPING_CASES)
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_against_the_twin(key, case):
    """m in {4, 12, 24}, correction on and off, 200 steps of a random amplitude table: modal coordinates per mode within 10 x the twin's defect plus the
    rounding of the device's own g_j (_mode_bars); every snapshot within ||  |X|^T dq ||_2 (dq: that bar per mode) + || expand_bound ||_2 (+ 10 rtol ||u_s|| max |a| for the static
    solve at rtol 1e-12); probes bit for bit the snapshot entries; energies against the twin's within the bound that follows from dq, dv."""
    f = H.load(key, "real")
    free = H.free_of(key)
    pv = np.array([free[0], free[len(free) // 2], free[-1], U.clamp_vars(key)[0]], dtype=np.int64)
    dt, amp = _load_case(key)
    c = _context(key)
    for m in (4, 12, 24):
        lam, X = _basis(key, m)
        c.set_modal_basis(lam, X, density=H.DENSITY)
        kw, (aR, bR, zeta) = _run_args(key, case, m)
        coef = M.modal_transient_coeffs(lam, T.mode_damping(lam, aR, bR, zeta), dt)
        g = X @ f
        defect, QL, VL = T.twin_defect(coef, g, amp, dt)
        dq = 10 * defect * np.abs(QL).max(axis=0).astype(np.float64)
        bq, bv = _mode_bars(X, f, g, defect, QL, VL, len(free))
        for corrected in (False, True):
            r = c.modal_transient(dt, N_STEPS, f, amp, static_correction=corrected, probes=pv, snapshot_stride=1, modal_coords=True, energies=True, **kw)
            assert r["info"]["staticSolves"] == int(corrected) and r["info"]["stepsDone"] == N_STEPS
            eq = T.rel_max(r["modal_coords"], QL)
            assert np.all(np.abs(r["modal_coords"] - QL).max(axis=0) <= bq), (m, corrected, eq, defect)
            assert np.array_equal(r["q"], r["modal_coords"][-1])
            assert np.all(np.abs(r["qdot"] - VL[-1]) <= bv)
            r_s = None
            B, Cm = X, QL.astype(np.float64).T
            if corrected:
                u_s = MU.static_solution(key, "real").real
                r_s = u_s - (g / lam) @ X
                B, Cm = np.vstack([X, r_s[None, :]]), np.vstack([Cm, amp[None, :]])
            ref = T.modal_fields(X, QL, r_s, amp)
            bar = np.linalg.norm(np.abs(X).T @ dq) + np.linalg.norm(MU.expand_bound(B, Cm), axis=1)
            if corrected:
                bar = bar + 10 * RTOL * np.linalg.norm(u_s) * np.abs(amp).max()
            err = np.linalg.norm(r["snapshots"] - ref, axis=1)
            print("%s %s m %d corrected %d: q %.3e of 10 x defect %.3e, snapshots %.3e of the bar" % (_name(key), case, m, corrected, eq / (10 * defect), defect, (err / bar).max()))
            assert r["snapshots"].shape == ref.shape and np.all(err <= bar)
            assert np.array_equal(r["probes"], r["snapshots"][:, pv])
            E = T.energies_of(lam, g, amp, QL, VL).astype(np.float64)
            Q, V = np.abs(QL).astype(np.float64), np.abs(VL).astype(np.float64)
            bars = (np.sum(V * bv + 0.5 * bv * bv, axis=1) + (m + 3) * EPS * E[:, 0], np.sum(lam * (Q * bq + 0.5 * bq * bq), axis=1) + (m + 4) * EPS * E[:, 1],
                    np.abs(amp) * (np.abs(g) @ bq + (m + 3) * EPS * (Q @ np.abs(g))))
            for col in range(3):
                assert np.all(np.abs(r["energies"][:, col] - E[:, col]) <= bars[col]), col
    c.close()


@pytest.mark.parametrize("case", T.DAMPING_CASES)
def test_full_basis_against_the_dense_exact_solution(case):
    """All 56 modes of the 2D linear mesh, the sampled sine: within 10 x the distance the float64 twin itself keeps from the dense exact solution
    (modal_transient_util.TWIN_DENSE_WORST, set and asserted by tests/test_modal_transient_reference.py), in that test's measure."""
    key = T.KEY56
    lam, X = MU.clamped_basis(key)
    assert len(lam) == 56
    f = H.load(key, "real")
    dt, amp = T.loads(key, N_STEPS)["sine"]
    kw, (aR, bR, zeta) = _run_args(key, case, 56)
    Ue = T.dense_exact(f, amp, dt, aR, bR, zeta)
    c = _context(key)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    r = c.modal_transient(dt, N_STEPS, f, amp, static_correction=False, snapshot_stride=1, **kw)
    c.close()
    dist = np.linalg.norm(r["snapshots"] - Ue, axis=1).max() / np.linalg.norm(Ue, axis=1).max()
    print("2D-P1 %s full basis against dense exact: %.3e (bar %.3e)" % (case, dist, 10 * T.TWIN_DENSE_WORST))
    assert dist <= 10 * T.TWIN_DENSE_WORST


# ---------------------------------------------------------------- individual properties
@pytest.mark.parametrize("key", [(2, 2), (3, 1)], ids=_name)
def test_constant_load_tends_to_the_static_solution(key):
    """Constant amplitude from rest, every mode critically or over-damped (aR = omega_1, bR = 1 / omega_1: decay rates >= omega_1 / 2), 200 steps of
    0.4 / omega_1: e^-40 of the transient is left, and with the correction u = sum phi_j g_j / lam_j + r_s = u_s: Context.solve at the same rtol up
    to the fma chains, 8 (m + 2) eps sum_j |g_j / lam_j| ||phi_j||_2 (the bar of the modal sweep's static limit) + 1e-16 for e^-40."""
    m = 12
    lam, X = _basis(key, m)
    f = H.load(key)
    w1 = float(np.sqrt(lam[0]))
    c = _context(key, options=(("deterministic", 1),))
    u = c.solve(f, rtol=RTOL, maxit=MAXIT)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    r = c.modal_transient(0.4 / w1, N_STEPS, f, damping=(w1, 1.0 / w1), rtol=RTOL, maxit=MAXIT, snapshot_stride=N_STEPS)
    c.close()
    q = (X @ f) / lam
    bar = (8 * (m + 2) * EPS + 1e-16) * (np.abs(q) @ np.linalg.norm(X, axis=1))
    err = np.linalg.norm(r["snapshots"][-1] - u)
    print("%s: static limit against solve %.3e (bar %.3e)" % (_name(key), err, bar))
    assert err <= bar


@pytest.mark.parametrize("key", [(2, 2), (3, 2)], ids=_name)
def test_free_vibration_of_a_mode_shape(key):
    """u0 = mode shape 2, no load, no damping: q_2(t) = cos omega_2 t, the others stay at their start values' size, E_kin + E_pot constant. Bar: the
    twin's defect x 10 plus what n steps of coefficients within 8 eps S can add to amplitude and phase, 16 n eps (the start values are the
    device's own projection)."""
    m, j = 12, 2
    lam, X = _basis(key, m)
    w = np.sqrt(lam)
    dt = 2.0 * np.pi / w[-1] / 12.0
    c = _context(key, options=(("deterministic", 1),))          # (the projection is made twice: the same bits only from the ordered sums)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    q0 = c.modal_coordinates(X[j])
    r = c.modal_transient(dt, N_STEPS, np.zeros(X.shape[1]), u0=X[j], static_correction=False, modal_coords=True, energies=True)
    c.close()
    assert np.array_equal(r["modal_coords"][0], q0) and abs(q0[j] - 1.0) <= 1e-12
    coef = M.modal_transient_coeffs(lam, 0.0, dt)
    defect, QL, _ = T.twin_defect(coef, np.zeros(m), np.zeros(N_STEPS + 1), dt, q0, np.zeros(m))
    bar = 10 * defect + 16 * N_STEPS * EPS
    t = dt * np.arange(N_STEPS + 1, dtype=np.longdouble)
    err = np.abs(r["modal_coords"][:, j] - q0[j] * np.cos(np.longdouble(w[j]) * t)).max()
    esum = r["energies"][:, 0] + r["energies"][:, 1]
    drift = np.abs(esum - esum[0]).max() / esum[0]
    print("%s: cos omega t %.3e, energy drift %.3e (bar %.3e)" % (_name(key), err, drift, bar))
    assert err <= bar and drift <= 2 * bar and np.all(r["energies"][:, 2] == 0.0)


@pytest.mark.parametrize("key", [(2, 1), (3, 2)], ids=_name)
def test_chaining_and_chunks_give_identical_bits(key):
    lam, X = _basis(key, 24)
    f = H.load(key)
    dt, amp = _load_case(key)
    pv = H.free_of(key)[[0, -1]]
    kw = dict(damping=H.damping(key, "rayleigh")[0], rtol=RTOL, maxit=MAXIT, probes=pv, modal_coords=True, energies=True, snapshot_stride=7)
    c = _context(key, options=(("deterministic", 1),))         # (every call makes its static solve: the same bits only from the ordered sums)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    one = c.modal_transient(dt, N_STEPS, f, amp, chunk_steps=32, **kw)
    assert one["info"]["chunkSteps"] == 32 and one["info"]["chunks"] == (N_STEPS + 1 + 31) // 32
    keys = ("q", "qdot", "probes", "modal_coords", "energies", "snapshots")
    for chunk in (64, 0):
        r = c.modal_transient(dt, N_STEPS, f, amp, chunk_steps=chunk, **kw)
        for k in keys:
            assert np.array_equal(r[k], one[k]), (chunk, k)
    cut = 77               # a multiple of the snapshot stride (the second call's snapshots are then the first's continued), no chunk edge
    a = c.modal_transient(dt, cut, f, amp[:cut + 1], chunk_steps=32, **kw)
    b = c.modal_transient(dt, N_STEPS - cut, f, amp[cut:], q0=a["q"], qdot0=a["qdot"], chunk_steps=32, **kw)
    c.close()
    for k in ("probes", "modal_coords", "energies"):
        assert np.array_equal(a[k], one[k][:cut + 1]) and np.array_equal(b[k], one[k][cut:]), k
    assert np.array_equal(a["snapshots"], one["snapshots"][:cut // 7 + 1]) and np.array_equal(b["snapshots"], one["snapshots"][cut // 7:])
    assert np.array_equal(b["q"], one["q"]) and np.array_equal(b["qdot"], one["qdot"])


def test_zero_steps_and_no_outputs():
    key = (2, 2)
    lam, X = _basis(key, 5)
    f = H.load(key)
    c = _context(key)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    q0, v0 = np.arange(1.0, 6.0), -np.arange(1.0, 6.0)
    r = c.modal_transient(0.1, 0, f, [2.0], q0=q0, qdot0=v0, static_correction=False, probes=[int(H.free_of(key)[3])], snapshot_stride=3, modal_coords=True, energies=True)
    assert np.array_equal(r["q"], q0) and np.array_equal(r["qdot"], v0) and np.array_equal(r["modal_coords"], q0[None, :])
    assert r["snapshots"].shape == (1, X.shape[1]) and np.array_equal(r["probes"][0], r["snapshots"][0, [H.free_of(key)[3]]])
    assert np.all(np.abs(r["snapshots"][0] - q0 @ X) <= MU.expand_bound(X, q0[:, None])[0])
    assert r["energies"].shape == (1, 3) and abs(r["energies"][0, 0] - 0.5 * v0 @ v0) <= 8 * EPS * (v0 @ v0)
    r = c.modal_transient(0.1, 40, f, static_correction=False)          # nothing asked for but the state
    assert r["probes"].shape == (41, 0) and r["snapshots"] is None and r["modal_coords"] is None and r["q"].any()
    c.close()


def test_free_body():
    """No fixed variables: the three M-orthonormalised rigid modes (lambda = 0) and 12 elastic modes against the twin; the correction is refused."""
    key = (2, 2)
    K, Mm = U.pencil(key)
    rM = H.DENSITY * Mm
    lam_all, X_all = U.free_truth(key, nev_max=15)[:2]
    Z = U.m_orthonormalise(U.rigid_modes(U.fem_mesh(key).node_pos), rM)
    lam = np.concatenate([np.zeros(3), lam_all[3:15] / H.DENSITY])
    X = np.concatenate([Z.T, X_all[:, 3:15].T / np.sqrt(H.DENSITY)])
    m = len(lam)
    f = H.load(key, "real", clamped=False)
    dt = 2.0 * np.pi / np.sqrt(lam[-1]) / 12.0
    amp = np.random.default_rng(29).standard_normal(N_STEPS + 1)
    c = _context(key, clamped=False)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    assert _code(lambda: c.modal_transient(dt, N_STEPS, f, amp, static_correction=True)) == _lib.ERR_UNSUPPORTED
    aR = 0.1 * float(np.sqrt(lam[3]))
    for damping in ((0.0, 0.0), (aR, 0.0)):
        r = c.modal_transient(dt, N_STEPS, f, amp, damping=damping, static_correction=False, modal_coords=True, snapshot_stride=10)
        coef = M.modal_transient_coeffs(lam, T.mode_damping(lam, *damping), dt)
        g = X @ f
        defect, QL, VL = T.twin_defect(coef, g, amp, dt)
        bq, _ = _mode_bars(X, f, g, defect, QL, VL, X.shape[1])
        eq = np.abs(r["modal_coords"] - QL).max(axis=0) / bq
        print("2D-P2 free, damping %s: q %.3e of the bar per mode, defect %.3e" % (damping, eq.max(), defect))
        assert np.all(np.isfinite(r["modal_coords"])) and np.all(eq <= 1.0)
        dq = 10 * defect * np.abs(QL).max(axis=0).astype(np.float64)
        Cm = QL.astype(np.float64).T[:, ::10]
        bar = np.linalg.norm(np.abs(X).T @ dq) + np.linalg.norm(MU.expand_bound(X, Cm), axis=1)
        assert np.all(np.linalg.norm(r["snapshots"] - T.modal_fields(X, QL)[::10], axis=1) <= bar)
    c.close()


# ---------------------------------------------------------------- refusals, state
def test_refusals():
    key = (3, 1)
    lam, X = _basis(key, 8)
    f = H.load(key)
    n = X.shape[1]
    c = _context(key)
    run = lambda n_steps=10, dt=0.1, amplitude=None, **kw: c.modal_transient(dt, n_steps, f, amplitude, **dict(dict(static_correction=False), **kw))
    assert _code(run) == _lib.ERR_STATE                                                                  # no basis
    set_ = lambda: c.set_modal_basis(lam, X, density=H.DENSITY)
    set_()
    first = run(modal_coords=True)
    for bad in (dict(dt=0.0), dict(dt=-0.1), dict(dt=float("nan")), dict(dt=float("inf")), dict(n_steps=-1), dict(snapshot_stride=-1), dict(damping=(-1.0, 0.0)),
                dict(damping=(0.0, -1.0)), dict(modal_damping=-0.01), dict(chunk_steps=-32), dict(chunk_steps=31), dict(chunk_steps=48), dict(probes=[n]),
                dict(probes=[-1]), dict(amplitude=[1.0] * 10 + [float("nan")]), dict(amplitude=[float("inf")] + [1.0] * 10),
                dict(static_correction=True, rtol=2.0), dict(static_correction=True, maxit=0)):
        assert _code(lambda: run(**bad)) == _lib.ERR_INVALID, bad
    prm = _lib.ModalTransientParams(0.1, 0.0, 0.0, 1e-8, 10, 100, 0, 0, 0, 0)
    info = _lib.ModalTransientInfo()
    q, qd, en, fp = np.zeros(8), np.zeros(8), np.zeros((11, 3)), _lib.ptr(np.ascontiguousarray(f))
    call = lambda p, q_, qd_, en_: c.lib.mfh_modal_transient(c.h, p, None, q_, qd_, fp, None, None, 0, None, None, None, en_, M.core.C.byref(info))
    ref = M.core.C.byref
    assert call(None, None, None, None) == _lib.ERR_INVALID                                               # null params
    assert call(ref(prm), _lib.ptr(q), None, None) == _lib.ERR_INVALID and call(ref(prm), None, _lib.ptr(qd), None) == _lib.ERR_INVALID     # one of q / qdot
    assert call(ref(prm), None, None, _lib.ptr(en)) == _lib.ERR_INVALID                                   # energies without the flag
    prm.flags = _lib.MODAL_TR_ENERGIES
    assert call(ref(prm), None, None, None) == _lib.ERR_INVALID                                           # the flag without the array
    prm.flags = 4
    assert call(ref(prm), None, None, None) == _lib.ERR_INVALID                                           # an unknown flag
    prm.flags = 0
    assert call(ref(prm), None, None, None) == _lib.OK
    with pytest.raises(ValueError):
        run(q0=np.zeros(8), u0=np.zeros(n))
    # staleness, by the rules of the basis
    c.set_density(np.full(c.n_elem, 2.0))
    assert _code(run) == _lib.ERR_STATE
    c.set_density(None)
    set_()
    c.fix_variables([int(H.free_of(key)[-1])])
    assert _code(run) == _lib.ERR_STATE
    c.clear_fixed()
    c.fix_variables(U.clamp_vars(key)[::-1].copy())
    assert np.array_equal(run(modal_coords=True)["modal_coords"], first["modal_coords"])
    # the static correction: a zero eigenvalue, a solve that does not converge (nothing written)
    lam0 = lam.copy()
    lam0[0] = 0.0
    c.set_modal_basis(lam0, X, density=H.DENSITY)
    assert _code(lambda: run(static_correction=True)) == _lib.ERR_INVALID
    run()
    set_()
    assert _code(lambda: run(static_correction=True, rtol=1e-12, maxit=1, probes=[int(H.free_of(key)[0])], modal_coords=True)) == _lib.ERR_NOT_CONVERGED
    last = c.last_modal_transient
    assert not last["probes"].any() and not last["modal_coords"].any() and not last["q"].any()
    c.close()


def test_nothing_existing_moves():
    """modal_harmonic (with its static correction, which shares the reserved columns of the basis) and newmark give the bits they gave before a
    transient run with correction, snapshots and energies."""
    key = (3, 2)
    c = _context(key, "multigrid", (("deterministic", 1),))
    f = H.load(key)
    lam, X = _basis(key, 12)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    w1 = float(np.sqrt(lam[0]))
    damping, _ = H.damping(key, "rayleigh")

    def snapshot():
        hr = c.modal_harmonic([0.0, 0.5 * w1], H.load(key, "complex"), damping=damping, rtol=1e-10, probes=H.free_of(key)[[0, -1]])
        nm = c.newmark(2.0 * np.pi / w1 / 20.0, 5, f=f, density=H.DENSITY, rtol=1e-10)
        return [hr["u"], hr["probes"], nm["u"], nm["v"], nm["a"], c.solve(f, rtol=1e-10)]
    before = snapshot()
    kw = dict(damping=damping, rtol=1e-10, snapshot_stride=5, energies=True, probes=[int(H.free_of(key)[1])])
    r = c.modal_transient(0.05 / w1, 64, f, **kw)
    assert r["info"]["staticSolves"] == 1
    after = snapshot()
    r2 = c.modal_transient(0.05 / w1, 64, f, **kw)
    c.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    for k in ("q", "qdot", "probes", "snapshots", "energies"):
        assert np.array_equal(r[k], r2[k]), k


# ---------------------------------------------------------------- end to end
def test_mid_mesh_against_newmark():
    """37 905 unknowns, clamped: modal_basis(30); a point force at a free variable with a half-sine history of 1.5 T_1, then free vibration under
    light Rayleigh damping; 2 000 steps at dt = T_1 / 100, two probes (the loaded variable and a neighbour). The modal run has no time error, so
    its distance from Context.newmark on the same context is Newmark's period error plus the truncation: over the first three periods (300 steps
    at dt against 150 at 2 dt -- the part of the run Newmark can follow at the cost of a test) it shrinks when both halve dt, and with the static
    correction -- which carries the local deformation under the point force, quasi-static for a pulse this slow -- it is below the uncorrected
    one."""
    key = U.MID
    c = _context(key, "jacobi", (("deterministic", 1),))       # (the corrected runs each make their static solve: the same bits only from the ordered sums)
    lam, X, info = c.modal_basis(30, density=H.DENSITY, batch=12, rtol=1e-6, maxit=3000)
    assert len(lam) == 30
    w = np.sqrt(lam)
    pv = H.free_of(key)[[-1, -2]]
    f = np.zeros(X.shape[1])
    f[pv[0]] = 1.0
    t1 = 2.0 * np.pi / w[0]
    aR, bR = 0.02 * w[0], 0.0
    dt = t1 / 100.0

    def history(h, steps):
        t = h * np.arange(steps + 1)
        return np.where(t < 1.5 * t1, np.sin(np.pi * t / (1.5 * t1)), 0.0)
    kw = dict(damping=(aR, bR), rtol=1e-10, maxit=MAXIT, probes=pv)
    r = c.modal_transient(dt, 2000, f, history(dt, 2000), energies=True, **kw)
    print("mid mesh: 2 000 steps, march %.2f ms, series %.2f ms, setup %.1f ms (%d static iterations), %d chunks" %
          (r["info"]["marchMs"], r["info"]["seriesMs"], r["info"]["setupMs"], r["info"]["staticIterations"], r["info"]["chunks"]))
    assert r["probes"].shape == (2001, 2) and np.all(np.isfinite(r["probes"])) and np.all(np.isfinite(r["energies"]))
    unc = c.modal_transient(dt, 2000, f, history(dt, 2000), static_correction=False, **kw)
    dist = {}
    for steps, h in ((150, 2 * dt), (300, dt)):
        amp = history(h, steps)
        nm = c.newmark(h, steps, f=f, amplitude=amp, density=H.DENSITY, damping=(aR, bR), rtol=1e-10, maxit=MAXIT, probes=pv)["probes"]
        mt = c.modal_transient(h, steps, f, amp, **kw)["probes"]
        mu = c.modal_transient(h, steps, f, amp, static_correction=False, **kw)["probes"]
        dist[steps] = (np.abs(mt - nm).max() / np.abs(nm).max(), np.abs(mu - nm).max() / np.abs(nm).max())
        if steps == 300:
            assert np.array_equal(mt, r["probes"][:301]) and np.array_equal(mu, unc["probes"][:301])
    c.close()
    print("mid mesh: against newmark, corrected / uncorrected: %.3e / %.3e at 2 dt, %.3e / %.3e at dt" % (dist[150] + dist[300]))
    assert dist[300][0] < dist[150][0]
    assert dist[300][0] < dist[300][1]
