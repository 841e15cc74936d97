"""mfh_mass_lumped_hrz, mfh_explicit_dt and mfh_explicit on the device against the numpy restatements of tests/explicit_util.py, on the small meshes
of tests/modes_util.py, its bar and (once) its mid mesh. Bars:
  lumped mass   (pairs of the DoF + 2) eps relative to the restatement on the kernel's own inputs (one rounding per product, per addition and for the
                density); independent of the library, against the restatement from the oracle alone: (pairs + 2 + 8 + 8) eps, the 8 and the 8 being the
                bars at which the library's weights and element volumes are first measured against the oracle's (test_lumped_mass)
  lambdaUpper   counted roundings, (npe dim + 2 pairs + 38) eps: 1.3e-14 on linear triangles, 3.6e-14 on quadratic tets (test_bounds)
  lambdaEst     100 x the largest float64-versus-longdouble defect of the numpy iteration over the fixtures, computed in the test (about 4e-16, the
                last digit depends on the host's numpy: a margin of about 4e-14)
  stepper       snapshots rel-L2 and energies relative to the column maximum against the longdouble recurrence: 10 x the float64 recurrence's own
                defect against it, measured per fixture and printed beside the value reached (docs/design/04_20_explicit_dynamics.md has the table)
  dispersion    10 x the float64 recurrence's own defect against phi cos(n theta); invariant drift: 10 x the float64 recurrence's own drift
  kernels       worst-case rounding bounds (each test states its own)
Every device run is made once (functools.lru_cache) and shared by the tests that look at it."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import meshfem_amd as M
from meshfem_amd import _lib

import explicit_util as X
import modes_util as U

pytestmark = pytest.mark.gpu

EPS = U.EPS
KEYS = list(U.SMALL) + [U.BAR]
name = X.name


def _context(key, options=(), clamped=True, device=0):
    V, T, deg, _ = U.mesh_arrays(key)
    c = M.Context(device)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    if clamped:
        c.fix_variables(U.clamp_vars(key))
    return c


def _probe_vars(key, clamped=True):
    free = X.free_of(key, clamped)
    return np.array([free[0], free[len(free) // 2], free[-1], free[0]], dtype=np.int64)


# ---------------------------------------------------------------- 1. lumped mass
W_EPS = 8       # the library's weights against the exact fractions: its mass table forms a vertex entry from four terms that cancel to a twelfth (4 eps reached)
V_EPS = 8       # the library's element volumes against the oracle's: the same differences of coordinates, then a determinant the device contracts into fmas (2 eps reached)


@pytest.mark.parametrize("key", KEYS, ids=name)
def test_lumped_mass(key):
    """Two comparisons. (a) The sum itself at the bar of (pairs + 2) eps: against the longdouble restatement fed the element volumes and weights the
    kernel is fed (one rounding per product, per addition and for the density). (b) Independent of the library: against the restatement from the
    oracle alone -- its volumes, the exact fractions of its Mref -- at (pairs + 2 + W_EPS + V_EPS) eps, the two inputs having been measured against
    the oracle's at W_EPS and V_EPS first. The total mass is compared with the oracle's volumes."""
    c = _context(key)
    assert np.array_equal(c.node_positions(), U.fem_mesh(key).node_pos)          # the oracle's node numbering is the library's own
    m = c.mass_lumped_hrz()
    again = c.mass_lumped_hrz()
    vol, w = c.elem_volumes(), c.debug_hrz_weights()
    exact = np.array([float(q) for q in X.exact_weights(key)])
    wdef, vdef = np.abs(w / exact - 1).max(), np.abs(vol / X.volumes(key) - 1).max()
    rho = X.element_density(key, 5)
    c.set_density(rho)
    mrho = c.mass_lumped_hrz()
    c.close()
    ref, pairs = X.lumped_mass(key, vol=vol, w=w)
    refrho, _ = X.lumped_mass(key, rho, vol=vol, w=w)
    ind, indrho = X.lumped_mass(key)[0], X.lumped_mass(key, rho)[0]
    err, errrho = np.abs(m / ref - 1).astype(np.float64), np.abs(mrho / refrho - 1).astype(np.float64)
    ierr, ierrrho = np.abs(m / ind - 1).astype(np.float64), np.abs(mrho / indrho - 1).astype(np.float64)
    print("%s: weights against the exact fractions %.2e (bar %d eps), volumes against the oracle's %.2e (bar %d eps); lumped mass against the restatement on the "
          "same inputs %.2e, with a density field %.2e (bar (pairs + 2) eps); against the oracle alone %.2e, %.2e, in units of its bar at most %.2f (pairs <= %d)" %
          (name(key), wdef, W_EPS, vdef, V_EPS, err.max(), errrho.max(), ierr.max(), ierrrho.max(),
           max((ierr / ((pairs + 2 + W_EPS + V_EPS) * EPS)).max(), (ierrrho / ((pairs + 2 + W_EPS + V_EPS) * EPS)).max()), pairs.max()))
    assert wdef <= W_EPS * EPS and abs(w.sum() - 1) <= 4 * EPS
    assert vdef <= V_EPS * EPS
    assert np.all(err <= (pairs + 2) * EPS) and np.all(errrho <= (pairs + 2) * EPS)
    assert np.all(ierr <= (pairs + 2 + W_EPS + V_EPS) * EPS) and np.all(ierrrho <= (pairs + 2 + W_EPS + V_EPS) * EPS)
    assert np.all(m > 0) and np.all(mrho > 0)
    assert np.array_equal(m, again)
    d = U.fem_mesh(key).N
    total, totalrho = d * X.volumes(key).sum(), d * (rho * X.volumes(key)).sum()
    assert abs(m.sum() - total) <= (np.sqrt(len(m)) + pairs.max() + 2 + W_EPS + V_EPS) * EPS * total
    assert abs(mrho.sum() - totalrho) <= (np.sqrt(len(m)) + pairs.max() + 2 + W_EPS + V_EPS) * EPS * totalrho
    assert np.array_equal(m.reshape(-1, d), np.repeat(m.reshape(-1, d)[:, :1], d, axis=1))


def test_row_sum_lumping_is_negative_where_hrz_is_positive():
    """Quadratic tets: mass_lumped returns negative vertex masses -- the reason explicit stepping was out of scope -- and HRZ does not."""
    c = _context((3, 2), clamped=False)
    hrz = c.mass_lumped_hrz()
    c.set_operator(M.OP_MASS)
    rows = c.mass_lumped()
    c.close()
    assert rows.min() < 0 < hrz.min()


# ---------------------------------------------------------------- 2. bounds
@functools.lru_cache(maxsize=None)
def _lambda_est_margin():
    worst = 0.0
    for key in KEYS:
        K = U.pencil(key)[0]
        for clamped in (True, False):
            args = (K, X.masses(key), X.fixed_of(key, clamped), X.default_start(K.shape[0]), 60)
            a, b = float(X.power_iteration(*args)), X.power_iteration(*args, X.LD)
            worst = max(worst, float(abs(a - b) / b))
    return 100.0 * worst


@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "free"])
@pytest.mark.parametrize("key", KEYS, ids=name)
def test_bounds(key, clamped):
    K = U.pencil(key)[0]
    fixed = X.fixed_of(key, clamped)
    c = _context(key, clamped=clamped)
    x0 = X.default_start(K.shape[0])
    given = c.explicit_dt(density=X.DENSITY, x0=x0)
    default = c.explicit_dt(density=X.DENSITY)
    short = c.explicit_dt(density=X.DENSITY, iters=7, x0=x0)
    c.close()
    c = _context(key, (("deterministic", 1),), clamped=clamped)      # (the K product of a default context adds in LDS in arrival order)
    det = [c.explicit_dt(density=X.DENSITY, x0=x0), c.explicit_dt(density=X.DENSITY), c.explicit_dt(density=X.DENSITY)]
    c.close()
    m = U.fem_mesh(key)
    # lambdaUpper against the restatement from the oracle's element matrices and masses, by counted roundings: an absolute row sum adds npe dim
    # terms and a DoF's sum its pairs on either side (one eps per term for the two together), the division and the scalar density 4, the mass below
    # it differs by at most its own independent bar (pairs + 2 + W_EPS + V_EPS) eps, and an entry of K_e formed by two formulas by 16 eps of its row's sum
    pairs_max = int(X.lumped_mass(key)[1].max())
    upper_bar = (m.nodes_per_elem * m.N + 2 * pairs_max + 6 + W_EPS + V_EPS + 16) * EPS
    upper = X.lambda_upper(key, fixed, X.DENSITY)
    est = float(X.power_iteration(K, X.masses(key), fixed, x0, 60))
    est7 = float(X.power_iteration(K, X.masses(key), fixed, x0, 7))
    lam_max = X.lambda_max(key, clamped)
    margin = _lambda_est_margin()
    print("%s %s: lambdaUpper %.3f lambda_max (against numpy %.2e, bar %.2e); lambdaEst %.5f lambda_max (against numpy %.2e, 7 steps %.2e, margin %.2e); %.2f ms" %
          (name(key), "clamped" if clamped else "free", given["lambdaUpper"] / lam_max, abs(given["lambdaUpper"] / upper - 1), upper_bar,
           given["lambdaEst"] / lam_max, abs(given["lambdaEst"] / est - 1), abs(short["lambdaEst"] / est7 - 1), margin, given["ms"]))
    assert abs(given["lambdaUpper"] / upper - 1) <= upper_bar
    assert abs(given["lambdaEst"] / est - 1) <= margin
    assert abs(short["lambdaEst"] / est7 - 1) <= margin and short["iterations"] == 7
    assert abs(default["lambdaEst"] / given["lambdaEst"] - 1) <= margin and default["iterations"] == 60
    assert det[0]["lambdaEst"] == det[1]["lambdaEst"] == det[2]["lambdaEst"]                    # the documented default start vector; the same bits
    assert det[0]["lambdaUpper"] == det[1]["lambdaUpper"] == given["lambdaUpper"] == default["lambdaUpper"]
    assert given["lambdaUpper"] >= lam_max >= given["lambdaEst"] * (1 - 64 * EPS)
    assert given["dtSafe"] == 2 / np.sqrt(given["lambdaUpper"]) and given["dtEst"] == 2 / np.sqrt(given["lambdaEst"])


# ---------------------------------------------------------------- 3. the stepper against the recurrence
def _run_case(c, key, case, n_steps=200, clamped=True, **kw):
    i = X.case_inputs(key, case, n_steps, clamped)
    args = dict(u0=i["u0"], v0=i["v0"], f=i["f"], amplitude=i["amplitude"], density=i["density"], damping=i["alpha"],
                probes=_probe_vars(key, clamped), snapshot_stride=1, energies=True)
    args.update(kw)
    return c.explicit(i["dt"], n_steps, **args)


@functools.lru_cache(maxsize=None)
def _device_run(key, case, clamped=True, options=(), n_steps=200):
    c = _context(key, options, clamped=clamped)
    r = _run_case(c, key, case, n_steps, clamped)
    c.close()
    return r


@functools.lru_cache(maxsize=None)
def _device_masses(key):
    """The recurrence runs on the masses the device returns, so that the stepper is compared on one and the same pencil. They are not taken on trust:
    test_lumped_mass holds them to (pairs + 2 + W_EPS + V_EPS) eps of the restatement from the oracle alone. A relative change of a mass by a few eps
    moves the phase of the highest modes by n omega dt / 2 times as much -- measured with the oracle's masses in the reference: up to 0.9 of the energy
    bar (0.4 on the same masses) and 18 times the bar of the final acceleration, which passes on the same masses -- so the comparison of schemes
    fixes that input."""
    c = _context(key, clamped=False)
    X.register_device_masses(key, c.mass_lumped_hrz())
    c.close()
    return "device"


def _check_against_reference(r, key, case, clamped, n_steps=200):
    src = _device_masses(key)
    Uld, Vld, Ald, Eld = X.reference_run(key, case, n_steps, clamped, X.LD, src)
    du, de = X.reference_defect(key, case, n_steps, clamped, src)
    err, eerr = X.rel_l2_rows(r["snapshots"], Uld), X.energy_defect(r["energies"], Eld)
    print("%s %s %s: snapshots %.3e (the recurrence's own defect %.3e, bar %.3e), energies %.3e (own defect %.3e, bar %.3e); dtEst / dt %.4f" %
          (name(key), case, "clamped" if clamped else "free", err, du, 10 * du, eerr, de, 10 * de, r["info"]["dtEst"] / X.case_inputs(key, case, n_steps, clamped)["dt"]))
    assert r["info"]["stepsDone"] == n_steps
    assert err <= 10 * du
    assert eerr <= 10 * de
    pv = _probe_vars(key, clamped)
    assert np.array_equal(r["probes"], r["snapshots"][:, pv])
    assert np.array_equal(r["u"], r["snapshots"][-1])
    _, V64, A64, _ = X.reference_run(key, case, n_steps, clamped, np.float64, src)
    assert X.rel_l2_rows(r["v"][None, :], Vld[-1:]) <= 10 * X.rel_l2_rows(V64, Vld)          # (the final state: the recurrence's own defect, over all steps)
    assert X.rel_l2_rows(r["a"][None, :], Ald[-1:]) <= 10 * X.rel_l2_rows(A64, Ald)
    fixed = X.fixed_of(key, clamped)
    assert np.all(r["snapshots"][:, fixed] == 0.0) and np.all(r["v"][fixed] == 0.0) and np.all(r["a"][fixed] == 0.0)


@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "free"])
@pytest.mark.parametrize("case", ["undamped", "damped"])
@pytest.mark.parametrize("key", KEYS, ids=name)
def test_against_the_recurrence(key, case, clamped):
    """200 steps at 0.9 dt_crit, a random load with a random amplitude table, non-zero u0 and v0, a snapshot and an energy row at every step."""
    _check_against_reference(_device_run(key, case, clamped), key, case, clamped)


def test_against_the_recurrence_mid():
    """The mid mesh (37 905 unknowns, quadratic tets: 75 workgroups of the step kernel) once: undamped, clamped, 50 steps -- the longdouble
    recurrence costs 30 ms a step there."""
    _check_against_reference(_device_run(U.MID, "undamped", True, (), 50), U.MID, "undamped", True, 50)


@pytest.mark.parametrize("j", [0, 3])
@pytest.mark.parametrize("key", KEYS, ids=name)
def test_dispersion_and_invariant(key, j):
    """Started from mode j of (K, M_L) at rest, no load: u_n = phi cos(n theta), sin(theta / 2) = omega dt / 2 -- independent of the recurrence, whose own
    defect against the closed form and own drift of the invariant are the units of the bars."""
    K = U.pencil(key)[0]
    lam, Phi = X.spectrum(key)
    phi, om = Phi[:, j], np.sqrt(lam[j])
    dt, n_steps = 0.9 * X.dt_crit(key), 200
    Us, _, _, E = X.explicit_direct(K, X.masses(key), X.fixed_of(key), dt, n_steps, phi, np.zeros_like(phi))
    closed = X.dispersion_closed_form(phi, om, dt, n_steps)
    own = np.linalg.norm(Us - closed, axis=1).max() / np.linalg.norm(phi)
    own_drift = np.abs(E[:, 3] / E[0, 3] - 1).max()
    c = _context(key)
    r = c.explicit(dt, n_steps, u0=phi, density=X.DENSITY, snapshot_stride=1, energies=True)
    c.close()
    err = np.linalg.norm(r["snapshots"] - closed, axis=1).max() / np.linalg.norm(phi)
    drift = np.abs(r["energies"][:, 3] / r["energies"][0, 3] - 1).max()
    print("%s mode %d: dispersion error %.3e (the recurrence's own %.3e), invariant drift %.3e (own %.3e)" % (name(key), j, err, own, drift, own_drift))
    assert err <= 10 * own
    assert drift <= 10 * own_drift


@pytest.mark.parametrize("key", KEYS, ids=name)
def test_damped_energy_never_increases(key):
    """Unloaded and damped, the invariant falls by aR dt v(n).M_L v(n) per step: it never increases (slack: 16 eps of its start value per step)."""
    i = X.case_inputs(key, "damped")
    c = _context(key)
    E = c.explicit(i["dt"], 200, u0=i["u0"], v0=i["v0"], density=i["density"], damping=i["alpha"], energies=True)["energies"]
    c.close()
    assert np.all(np.diff(E[:, 3]) <= 16 * EPS * E[0, 3])
    assert E[-1, 3] < E[0, 3]
    loss = -np.diff(E[:, 3])
    want = i["alpha"] * i["dt"] * 2.0 * E[1:, 0]
    assert np.abs(loss - want).max() <= 1e-10 * E[0, 3]


@pytest.mark.parametrize("key", KEYS, ids=name)
def test_free_body_keeps_its_momentum(key):
    """Free and unloaded: sum_d m_d v_d per component stays at its start value (the rows of K sum to zero); bar: 10 x the float64 recurrence's drift."""
    i = X.case_inputs(key, "undamped", 200, False)
    d = U.fem_mesh(key).N
    mass = X.masses(key)
    c = _context(key, clamped=False)
    r = c.explicit(i["dt"], 200, u0=i["u0"], v0=i["v0"], density=i["density"])
    c.close()
    Vref = X.explicit_direct(U.pencil(key)[0], mass, X.fixed_of(key, False), i["dt"], 200, i["u0"], i["v0"])[1]
    scale = np.abs(mass * i["v0"]).sum()
    p0 = (mass * i["v0"]).reshape(-1, d).sum(axis=0)
    own = np.abs((mass * Vref[-1]).reshape(-1, d).sum(axis=0) - p0).max() / scale
    drift = np.abs((mass * r["v"]).reshape(-1, d).sum(axis=0) - p0).max() / scale
    print("%s: momentum drift %.3e (the recurrence's own %.3e)" % (name(key), drift, own))
    assert drift <= 10 * max(own, EPS)


@pytest.mark.parametrize("key", [(2, 2), (3, 2)], ids=name)
def test_chained_calls_equal_one_run(key):
    """50 + 50 steps chained through (u, v, a) equal 100 steps bit for bit under option deterministic, and a second run equals the first."""
    i = X.case_inputs(key, "damped")
    c = _context(key, (("deterministic", 1),))
    common = dict(f=i["f"], density=i["density"], damping=i["alpha"], snapshot_stride=1, energies=True)
    whole = c.explicit(i["dt"], 100, u0=i["u0"], v0=i["v0"], amplitude=i["amplitude"][:101], **common)
    again = c.explicit(i["dt"], 100, u0=i["u0"], v0=i["v0"], amplitude=i["amplitude"][:101], **common)
    first = c.explicit(i["dt"], 50, u0=i["u0"], v0=i["v0"], amplitude=i["amplitude"][:51], **common)
    second = c.explicit(i["dt"], 50, u0=first["u"], v0=first["v"], a0=first["a"], amplitude=i["amplitude"][50:101], **common)
    c.close()
    for k in ("u", "v", "a", "snapshots", "energies"):
        assert np.array_equal(whole[k], again[k])
    assert np.array_equal(first["snapshots"], whole["snapshots"][:51]) and np.array_equal(second["snapshots"], whole["snapshots"][50:])
    assert np.array_equal(first["energies"], whole["energies"][:51]) and np.array_equal(second["energies"], whole["energies"][50:])
    for k in ("u", "v", "a"):
        assert np.array_equal(second[k], whole[k])


def test_strides():
    """snapshot_stride 7 and energy_stride 5 pick the rows of the stride-1 run."""
    key = (3, 1)
    full = _device_run(key, "damped", True, (("deterministic", 1),))
    c = _context(key, (("deterministic", 1),))
    r = _run_case(c, key, "damped", snapshot_stride=7, energy_stride=5)
    c.close()
    assert np.array_equal(r["snapshots"], full["snapshots"][::7]) and np.array_equal(r["energies"], full["energies"][::5])
    assert np.array_equal(r["probes"], full["probes"]) and np.array_equal(r["u"], full["u"])


# ---------------------------------------------------------------- 4. step-size policy
@pytest.mark.parametrize("key", U.SMALL, ids=name)
def test_step_size_policy(key):
    K = U.pencil(key)[0]
    i = X.case_inputs(key, "undamped")
    c = _context(key)
    with pytest.raises(_lib.MeshFEMHipError) as e:
        c.explicit(1.05 * X.dt_crit(key), 10, u0=i["u0"], density=i["density"])
    assert e.value.code == _lib.ERR_INVALID and c.last_explicit["info"]["dtEst"] < 1.05 * X.dt_crit(key)
    # the same step unchecked: the growth factor is 1.88 per step, the overflow is certain within 2 000 steps
    u0 = i["u0"].copy()
    with pytest.raises(_lib.MeshFEMHipError) as e:
        c.explicit(1.05 * X.dt_crit(key), 2000, u0=u0, density=i["density"], check_dt=False)
    assert e.value.code == _lib.ERR_NOT_CONVERGED
    done = c.last_explicit["info"]["stepsDone"]
    print("%s: blow-up noticed, stepsDone %d" % (name(key), done))
    assert done == 0 or (done < 2000 and done % 256 == 255)
    assert np.array_equal(c.last_explicit["u"], u0)
    # the context is as good as before: the next solve is correct
    free = X.free_of(key)
    f = np.zeros(K.shape[0])
    f[free] = np.random.default_rng(3).standard_normal(len(free))
    u = c.solve(f, rtol=1e-12)
    c.close()
    ref = np.zeros_like(f)
    ref[free] = spla.spsolve(K[free][:, free].tocsc(), f[free])
    assert np.linalg.norm(u - ref) <= 1e-9 * np.linalg.norm(ref)


# ---------------------------------------------------------------- 5. the kernels alone
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 100003])
def test_step_kernel(n):
    """k_explicit_step through its hook under dyn_grid_cap 1 (one workgroup: the lanes loop), every mode, last and not. Per value the bar is 8 eps of the
    sum of the magnitudes of the terms it is formed from; an energy sum gets (n / 512 + 32) eps of the sum of the magnitudes of its terms (a lane
    adds at most n / 512 + 1 terms one after the other, the tree adds 8 levels)."""
    rng = np.random.default_rng(n)
    c = M.Context(0)
    c.set_option("dyn_grid_cap", 1)
    y, u, v, f, a = (rng.standard_normal(n) for _ in range(5))
    mass = 0.5 + rng.random(n)
    inv = 1.0 / mass
    inv[rng.random(n) < 0.1] = 0.0
    dt, alpha, g = 0.37, 0.8, -1.3
    probes = np.array([0, n - 1, n // 2, 0], dtype=np.int64)
    L = X.LD
    yl, ul, vl, fl, al, ml, il = (x.astype(L) for x in (y, u, v, f, a, mass, inv))
    hdt, den = L(dt) / 2, 1 + L(alpha) * L(dt) / 2
    for mode in (0, 1, 2):
        for last in (0, 1):
            r = c.debug_explicit_step(dt, alpha, g, mode, last, y, u, v, inv, mass=mass, f=f, a=a, probes=probes)
            if mode == 0:
                ak = (il * (L(g) * fl - yl) - L(alpha) * vl) / den
                ak_mag = (np.abs(il) * (abs(g) * np.abs(fl) + np.abs(yl)) + alpha * np.abs(vl)) / den
                vk, vk_mag = vl + hdt * ak, np.abs(vl) + hdt * ak_mag
            else:
                ak = al if mode == 2 else il * (L(g) * fl - yl) - L(alpha) * vl
                ak_mag = np.abs(al) if mode == 2 else np.abs(il) * (abs(g) * np.abs(fl) + np.abs(yl)) + alpha * np.abs(vl)
                vk, vk_mag = vl, np.abs(vl)
            vh, vh_mag = vk + hdt * ak, vk_mag + hdt * ak_mag
            un, un_mag = ul + L(dt) * vh, np.abs(ul) + dt * vh_mag
            assert r["flag"] == 0
            assert np.array_equal(r["snapshot"], u) and np.array_equal(r["probes"], u[probes])
            if last:
                assert np.array_equal(r["u"], u)
                assert np.all(np.abs(r["v"] - vk) <= 8 * EPS * vk_mag) and np.all(np.abs(r["a"] - ak) <= 8 * EPS * ak_mag)
            else:
                assert np.all(np.abs(r["u"] - un) <= 8 * EPS * un_mag) and np.all(np.abs(r["v"] - vh) <= 8 * EPS * vh_mag)
                assert np.array_equal(r["a"], a)
            terms = [ml * vk * vk / 2, ul * yl / 2, L(g) * fl * ul, (ml * vh * vh + un * yl) / 2]
            mags = [ml * vk_mag ** 2 / 2, np.abs(ul * yl) / 2, abs(g) * np.abs(fl * ul), (ml * vh_mag ** 2 + un_mag * np.abs(yl)) / 2]
            for k in range(4):
                assert abs(r["energies"][k] - terms[k].sum()) <= (n / 512 + 32) * EPS * float(mags[k].sum()), (n, mode, last, k)
    # a value that is not finite raises the flag, whichever lane meets it
    bad = u.copy()
    bad[n - 1] = np.inf
    assert c.debug_explicit_step(dt, alpha, g, 0, 0, y, bad, v, inv, mass=mass, f=f)["flag"] == 1
    big = np.full(n, 1.7e308)
    assert c.debug_explicit_step(dt, alpha, g, 0, 0, y, big, big, inv, mass=mass, f=f)["flag"] == 1
    c.close()


ROW_SUM_CASES = [(k, "iso") for k in KEYS] + [((2, 2), "ortho_field"), ((3, 1), "general"), ((3, 2), "ortho_field"), ((3, 2), "general_field"), ((2, 1), "general_field")]


@pytest.mark.parametrize("key,mode", ROW_SUM_CASES, ids=lambda v: v if isinstance(v, str) else name(v))
def test_element_row_sums(key, mode):
    """k_elem_abs_rowsums under dyn_grid_cap 1 against the oracle's element matrices, in every material flavour the kernel is instantiated for
    (isotropic, orthotropic, general; constant and per element). Bar by counted roundings: npe dim terms added on either side (one eps per term for
    the two) and an entry formed by two formulas to 16 eps of its row's sum: (npe dim + 16) eps."""
    import element_integrals_util as EI
    c = _context(key, (("dyn_grid_cap", 1),))
    if mode != "iso":
        EI.material(mode, U.fem_mesh(key).N, len(U.mesh_arrays(key)[1]))[0](c)
    rs = c.debug_elem_abs_rowsums()
    c.close()
    ref = X.elem_abs_rowsums(key, mode)
    m = U.fem_mesh(key)
    err = np.abs(rs / ref - 1).max()
    bar = (m.nodes_per_elem * m.N + 16) * EPS
    print("%s %s: element row sums %.2e (bar %.2e)" % (name(key), mode, err, bar))
    assert err <= bar


def test_stepper_under_one_workgroup():
    """dyn_grid_cap 1 on the quadratic tets: the lanes of every new kernel loop; the run still meets the bars of the recurrence."""
    key = (3, 2)
    _check_against_reference(_device_run(key, "damped", True, (("dyn_grid_cap", 1),)), key, "damped", True)
    c = _context(key, (("dyn_grid_cap", 1),))
    one = c.explicit_dt(density=X.DENSITY)
    m1 = c.mass_lumped_hrz()
    c.close()
    c = _context(key)
    many = c.explicit_dt(density=X.DENSITY)
    m2 = c.mass_lumped_hrz()
    c.close()
    assert np.array_equal(m1, m2) and one["lambdaUpper"] == many["lambdaUpper"]
    assert abs(one["lambdaEst"] / many["lambdaEst"] - 1) <= _lambda_est_margin()


# ---------------------------------------------------------------- 6. nothing existing moves
@pytest.mark.parametrize("storage", [-1, 0], ids=["default-storage", "both-triangles"])
def test_nothing_existing_moves(storage):
    """Under deterministic: mfh_solve, mfh_newmark (10 steps) and mfh_modes give the same bits before and after an explicit run on the context."""
    key = (3, 2)
    i = X.case_inputs(key, "damped")
    options = (("deterministic", 1),) + ((("matrix_storage", 0),) if storage == 0 else ())
    c = _context(key, options)
    free = X.free_of(key)
    f = np.zeros(len(i["f"]))
    f[free] = np.random.default_rng(4).standard_normal(len(free))

    def existing():
        u = c.solve(f, rtol=1e-10)
        nm = c.newmark(0.05, 10, u0=i["u0"], v0=i["v0"], f=i["f"], density=i["density"], rtol=1e-10, snapshot_stride=1)
        lam, Xm, _ = c.modes(3, density=i["density"])
        return u, nm["snapshots"], nm["v"], lam, Xm
    before = existing()
    r = _run_case(c, key, "damped")
    dt_info = c.explicit_dt(density=i["density"])
    c.mass_lumped_hrz()
    after = existing()
    c.close()
    assert r["info"]["stepsDone"] == 200 and dt_info["lambdaEst"] > 0
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    if storage == -1:
        assert np.array_equal(r["snapshots"], _device_run(key, "damped", True, (("deterministic", 1),))["snapshots"])


# ---------------------------------------------------------------- 7. refusals
def _raw_explicit(c, dt=0.01, density=1.0, alpha=0.0, n_steps=2, snap=0, estride=0, flags=0, probes=None, energies=False, snapshots=False):
    n = c.bs * c.n_dof
    u, v, a = np.zeros(n), np.zeros(n), np.zeros(n)
    prm = _lib.ExplicitParams(dt, density, alpha, n_steps, snap, estride, flags)
    pv = None if probes is None else np.asarray(probes, dtype=np.int64)
    pout = None if probes is None else np.zeros((max(n_steps, 0) + 1, len(pv)))
    en = np.zeros((max(n_steps, 0) + 1, 4)) if energies else None
    sn = np.zeros((max(n_steps, 0) + 1, n)) if snapshots else None
    info = _lib.ExplicitInfo()
    p = _lib.ptr
    return c.lib.mfh_explicit(c.h, C.byref(prm), p(u), p(v), p(a), None, None, p(pv), 0 if pv is None else len(pv), p(pout), p(sn), p(en), C.byref(info))


@pytest.mark.parametrize("device", [0, -1], ids=["device", "host-only"])
def test_refusals(device):
    """MFH_ERR_INVALID before any device work, so a host-only context refuses the same way."""
    key = (2, 1)
    c = _context(key, device=device)
    n = c.bs * c.n_dof
    bad = [dict(dt=0.0), dict(dt=-1.0), dict(dt=np.nan), dict(density=0.0), dict(density=-2.0), dict(alpha=-0.1), dict(n_steps=-1), dict(snap=-1), dict(estride=-1),
           dict(flags=8), dict(probes=[n]), dict(probes=[-1]), dict(energies=True), dict(flags=_lib.EXP_ENERGIES), dict(snapshots=True)]
    for kw in bad:
        assert _raw_explicit(c, **kw) == _lib.ERR_INVALID, kw
    info = _lib.ExplicitDtInfo()
    assert c.lib.mfh_explicit_dt(c.h, 0.0, 0, None, C.byref(info)) == _lib.ERR_INVALID
    assert c.lib.mfh_explicit_dt(c.h, 1.0, -1, None, C.byref(info)) == _lib.ERR_INVALID
    assert c.lib.mfh_explicit_dt(c.h, 1.0, 0, None, None) == _lib.ERR_INVALID
    out = np.zeros(n)
    assert c.lib.mfh_mass_lumped_hrz(c.h, _lib.ptr(out), 4) == _lib.ERR_INVALID
    assert c.lib.mfh_mass_lumped_hrz(c.h, None, 0) == _lib.ERR_INVALID
    if device == -1:
        assert _raw_explicit(c) == _lib.ERR_HIP                               # valid arguments: no device, and there is no CPU fallback
        assert c.lib.mfh_mass_lumped_hrz(c.h, _lib.ptr(out), 0) == _lib.ERR_STATE   # (as mfh_mass_apply refuses it)
    else:
        assert _raw_explicit(c) == _lib.OK
        # a start vector without a free component
        assert c.lib.mfh_explicit_dt(c.h, 1.0, 0, _lib.ptr(np.zeros(n)), C.byref(info)) == _lib.ERR_INVALID
        # no free variable: the dt check has no estimate to check against and says so, as mfh_explicit_dt does; unchecked, the run is trivial
        c.clear_fixed()
        c.fix_variables(np.arange(n))
        assert _raw_explicit(c) == _lib.ERR_INVALID and "Rayleigh quotient" in c.lib.mfh_last_error(c.h).decode()
        assert c.lib.mfh_explicit_dt(c.h, 1.0, 0, None, C.byref(info)) == _lib.ERR_INVALID
        assert _raw_explicit(c, flags=_lib.EXP_NO_DT_CHECK) == _lib.OK
        c.set_operator(M.OP_LAPLACIAN)
        assert c.lib.mfh_explicit_dt(c.h, 1.0, 0, None, C.byref(info)) == _lib.ERR_UNSUPPORTED       # contexts as for mfh_newmark
    c.close()
