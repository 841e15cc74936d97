"""mfh_harmonic on the device against the complex direct solves of tests/harmonic_util.py, on the small meshes of tests/modes_util.py and on its mid
mesh. rtol = 1e-12. Bars, set against the CPU stand-in of the loop (tests/test_harmonic_reference.py: a numpy COCG lands within 66 rtol of the direct
solve and its true residual within 44 rtol), not against the device's own output:
  fields          rel-L2 over both planes <= 1e3 rtol against the direct solve (the convention of tests/test_gpu_dynamics.py)
  true residuals  <= 1e2 rtol
  probes          equal to the field entries bit for bit
  undamped, real load: the imaginary plane is exactly zero
  product         componentwise worst-case rounding bound (the test states it)
Every device run is made once (functools.lru_cache) and shared by the tests that look at it."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import meshfem_amd as M
from meshfem_amd import _lib

import harmonic_util as H
import modes_util as U

pytestmark = pytest.mark.gpu

RTOL = 1e-12
BAR = 1e3 * RTOL
EPS = U.EPS
PRECONDS = {"jacobi": M.PRECOND_BLOCK_JACOBI, "two-level": M.PRECOND_TWO_LEVEL, "multigrid": M.PRECOND_MULTIGRID}
MAXIT = 20000


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
    free = H.free_of(key, clamped)
    return np.array([free[0], free[len(free) // 2], free[-1], free[0]], dtype=np.int64)


def _sweep(c, key, case, omegas=None, kind="real", clamped=True, **kw):
    damping, eta = H.damping(key, case, clamped)
    args = dict(density=H.DENSITY, damping=damping, loss_factor=eta, rtol=RTOL, maxit=MAXIT, probes=_probe_vars(key, clamped))
    args.update(kw)
    return c.harmonic(H.sweep_omegas(key) if omegas is None else omegas, H.load(key, kind, clamped), **args)


@functools.lru_cache(maxsize=None)
def _device_run(key, case, precond, options=()):
    c = _context(key, precond, options)
    assert np.array_equal(c.node_positions(), U.fem_mesh(key).node_pos)          # the oracle's node numbering is the library's own
    r = _sweep(c, key, case)
    c.close()
    return r


def _worst_error(u, ref):
    return max(H.rel_l2(u[k], ref[k]) for k in range(len(ref)))


REFERENCE_CASES = [(k, p) for k in U.SMALL for p in ("jacobi", "two-level", "multigrid")]


@pytest.mark.parametrize("case", list(H.CASES))
@pytest.mark.parametrize("key,precond", REFERENCE_CASES, ids=_name)
def test_against_the_direct_solve(key, precond, case):
    """One call of the five test frequencies (0, omega_1 / 2 and three midpoints between natural frequencies), every preconditioner, undamped,
    Rayleigh-damped (0.1 omega_1, 0.02 / omega_1) and with the structural loss factor 0.03."""
    r = _device_run(key, case, precond)
    ref = H.reference(key, case)
    info = r["info"]
    err, res = _worst_error(r["u"], ref), float(r["true_residuals"].max())
    print("%s %s %s: error %.3e (bar %.1e), true residual %.3e (bar %.1e), iterations %s, note '%s'" %
          (_name(key), case, precond, err, BAR, res, 1e2 * RTOL, list(r["iterations"]), info["note"]))
    assert info["freqsDone"] == H.N_FREQ
    assert err <= BAR
    assert res <= 1e2 * RTOL and info["worstTrueResidual"] == res
    assert info["iterationsTotal"] == r["iterations"].sum() and info["iterationsMax"] == r["iterations"].max()
    pv = _probe_vars(key)
    assert np.array_equal(r["probes"], r["u"][:, pv])
    fixed = U.clamp_vars(key)
    assert np.all(r["u"][:, fixed] == 0.0)
    if case == "undamped":
        assert np.all(r["u"].imag == 0.0)                     # a real system stays real: exactly (+-0)
    want, used = PRECONDS[precond], info["precondUsed"]
    if key == (3, 2):
        assert used == want                                   # both hierarchies build on the quadratic tets: the two-level and the V-cycle path ran
    elif used != want:
        assert info["note"]                                   # the hierarchy does not apply to this mesh: the note says what ran instead
        assert used == M.PRECOND_BLOCK_JACOBI and "block-Jacobi" in info["note"]


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_static_limit(key):
    """omega = 0, undamped, real load: the solution of Context.solve on the same context."""
    c = _context(key, "multigrid")
    f = H.load(key)
    r = c.harmonic([0.0], f, density=H.DENSITY, rtol=RTOL, maxit=MAXIT)
    u = c.solve(f, rtol=RTOL, maxit=MAXIT)
    c.close()
    err = H.rel_l2(r["u"][0].real, u)
    print("%s: omega = 0 against solve %.3e" % (_name(key), err))
    assert err <= BAR
    assert np.all(r["u"].imag == 0.0)


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_complex_loads(key):
    """f^ = i g against i x (the response to g); a load with both planes random against the direct solve. Rayleigh case."""
    c = _context(key, "multigrid")
    g = H.load(key)
    r1 = _sweep(c, key, "rayleigh")
    r2 = c.harmonic(H.sweep_omegas(key), 1j * g, density=H.DENSITY, damping=H.damping(key, "rayleigh")[0], rtol=RTOL, maxit=MAXIT)
    r3 = _sweep(c, key, "rayleigh", kind="complex")
    c.close()
    e2 = _worst_error(r2["u"], 1j * r1["u"])
    e3 = _worst_error(r3["u"], H.reference(key, "rayleigh", "complex"))
    print("%s: i g against i u(g) %.3e, complex load against the direct solve %.3e" % (_name(key), e2, e3))
    assert e2 <= BAR and e3 <= BAR


@pytest.mark.parametrize("case", ["rayleigh", "structural"])
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_dissipation_identity(key, case):
    """Im(u^H f) = w (aR u^H M u + bR u^H K u) + eta u^H K u with M u and K u from mass_apply / apply_K: no oracle involved."""
    r = _device_run(key, case, "multigrid")
    (aR, bR), eta = H.damping(key, case)
    f = H.load(key)
    c = _context(key, "multigrid")
    worst = 0.0
    for k, w in enumerate(H.sweep_omegas(key)):
        u = r["u"][k]
        Ku = c.apply_K(np.ascontiguousarray(u.real)) + 1j * c.apply_K(np.ascontiguousarray(u.imag))
        Mu = H.DENSITY * (c.mass_apply(np.ascontiguousarray(u.real)) + 1j * c.mass_apply(np.ascontiguousarray(u.imag)))
        uKu, uMu = np.vdot(u, Ku).real, np.vdot(u, Mu).real
        lhs, rhs = np.vdot(u, f).imag, w * (aR * uMu + bR * uKu) + eta * uKu
        worst = max(worst, abs(lhs - rhs) / abs(np.vdot(u, f)))
    c.close()
    print("%s %s: dissipation identity %.3e of |u^H f|" % (_name(key), case, worst))
    assert worst <= BAR


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_sweep_through_the_first_resonance(key):
    """21 frequencies across [0.8, 1.2] omega_1, Rayleigh case, warm start on and off."""
    w1 = float(H.natural_frequencies(key)[0])
    om = tuple(np.linspace(0.8 * w1, 1.2 * w1, 21))
    ref = H.reference(key, "rayleigh", "real", om)
    c = _context(key, "multigrid")
    on = _sweep(c, key, "rayleigh", omegas=om)
    off = _sweep(c, key, "rayleigh", omegas=om, warm_start=False)
    c.close()
    e_on, e_off = _worst_error(on["u"], ref), _worst_error(off["u"], ref)
    e_x = _worst_error(on["u"], off["u"])
    print("%s: warm %.3e (%d iterations), cold %.3e (%d iterations), warm against cold %.3e" %
          (_name(key), e_on, on["info"]["iterationsTotal"], e_off, off["info"]["iterationsTotal"], e_x))
    assert e_on <= BAR and e_off <= BAR and e_x <= BAR


@pytest.mark.parametrize("key", [(2, 2), (3, 1)], ids=_name)
def test_free_body(key):
    """No fixed variables: block-Jacobi whatever the context's preconditioner; omega between the first two distinct non-zero free frequencies.
    omega = 0 is refused."""
    w = H.natural_frequencies(key, clamped=False)
    second = w[np.nonzero(w > w[0] * (1 + 1e-6))[0][0]]
    om = (0.5 * (float(w[0]) + float(second)),)
    c = _context(key, "multigrid", clamped=False)
    for case in ("undamped", "rayleigh"):
        r = _sweep(c, key, case, omegas=om, clamped=False)
        err = _worst_error(r["u"], H.reference(key, case, "real", om, False))
        print("%s free %s: error %.3e, %d iterations, note '%s'" % (_name(key), case, err, r["iterations"][0], r["info"]["note"]))
        assert err <= BAR
        assert r["info"]["precondUsed"] == M.PRECOND_BLOCK_JACOBI and "no fixed variables" in r["info"]["note"]
    with pytest.raises(M.MeshFEMHipError) as ei:
        _sweep(c, key, "undamped", omegas=(0.0,), clamped=False)
    assert ei.value.code == _lib.ERR_INVALID
    c.close()


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


@pytest.mark.parametrize("two_pass", [0, 1], ids=["one-pass", "two-pass"])
@pytest.mark.parametrize("cap", [1, 2048])
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_complex_pencil_product(key, cap, two_pass):
    """mfh_debug_harmonic_apply against scipy, masked and not, one workgroup (the lanes loop) and the default grid, the single-pass kernel and the
    two-launch form: |y - Z x| <= 4 L eps (|zK| |K| + |zM| |M|) |x| componentwise (L the longest row: the sums of the two products and the
    complex combination, each complex product two roundings), and x^T y to the sum of the same bound."""
    K, Mm = _device_pencil(key)
    n = K.shape[0]
    rng = np.random.default_rng(5)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    zK, zM = complex(1.0, 0.37), complex(-2.3, 0.61)
    L = int(np.diff(K.indptr).max())
    c = _context(key, "jacobi", (("dyn_grid_cap", cap), ("harmonic_two_pass", two_pass)))
    fixed = U.clamp_vars(key)
    for masked in (False, True):
        xm = x.copy()
        if masked:
            xm[fixed] = 0.0
        y, dot = c.debug_harmonic_apply(zK, zM, xm, masked)
        ref = zK * (K @ xm) + zM * (Mm @ xm)
        bound = 4 * L * EPS * (abs(zK) * (abs(K) @ np.abs(xm)) + abs(zM) * (abs(Mm) @ np.abs(xm)))
        if masked:
            ref[fixed] = 0.0
            assert np.all(y[fixed] == 0.0)
        worst = (np.abs(y - ref) / np.where(bound > 0, bound, 1.0)).max()
        print("%s cap %d two-pass %d masked %d: worst error / bound %.3e" % (_name(key), cap, two_pass, masked, worst))
        assert np.all(np.abs(y - ref) <= bound)
        assert abs(dot - xm @ y) <= (n + 4) * EPS * (np.abs(xm) @ np.abs(y))      # the unconjugated x^T y of the kernel's own y, any summation order
    yM, _ = c.debug_harmonic_apply(0.0, zM, x, False)         # zK == 0: the K products are skipped, y is not read
    refM = zM * (Mm @ x)
    assert np.all(np.abs(yM - refM) <= 4 * L * EPS * abs(zM) * (abs(Mm) @ np.abs(x)))
    c.close()


@pytest.mark.parametrize("options", [(("dyn_grid_cap", 1),), (("harmonic_two_pass", 1),)], ids=["cap-1", "two-pass"])
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_loop_past_its_cap_and_in_two_passes(key, options):
    """A full 5-frequency run with one workgroup per kernel (every lane loops), and with the two-launch form of the mass product."""
    for precond in ("jacobi", "multigrid"):
        r = _device_run(key, "rayleigh", precond, options)
        err = _worst_error(r["u"], H.reference(key, "rayleigh"))
        print("%s %s %s: error %.3e" % (_name(key), precond, options, err))
        assert err <= BAR and r["true_residuals"].max() <= 1e2 * RTOL


@pytest.mark.parametrize("key", [(2, 2), (3, 2)], ids=_name)
def test_deterministic(key):
    c = _context(key, "multigrid", (("deterministic", 1),))
    a = _sweep(c, key, "rayleigh")
    b = _sweep(c, key, "rayleigh")
    c.close()
    assert np.array_equal(a["u"], b["u"]) and np.array_equal(a["iterations"], b["iterations"])
    assert np.array_equal(a["true_residuals"], b["true_residuals"])


def test_maxit_stops_the_sweep():
    """maxit = 2 on a 3-frequency call: MFH_ERR_NOT_CONVERGED, freqsDone = the leading frequencies a full run finishes within 2 iterations, their
    rows equal to the full run's, the rest untouched."""
    key = (3, 2)
    om = H.sweep_omegas(key)[:3]
    c = _context(key, "multigrid")
    full = _sweep(c, key, "rayleigh", omegas=om)
    expect = 0
    while expect < 3 and full["iterations"][expect] <= 2:
        expect += 1
    assert expect < 3
    n = c.bs * c.n_dof
    damping, eta = H.damping(key, "rayleigh")
    prm = _lib.HarmonicParams(H.DENSITY, damping[0], damping[1], eta, RTOL, 3, 2, _lib.HARM_WARM_START)
    f = np.ascontiguousarray(H.load(key))
    pv = _probe_vars(key)
    fld, pout = np.full((3, 2, n), 7.0), np.full((3, len(pv), 2), 7.0)
    its, res = np.full(3, -5, dtype=np.int32), np.full(3, 7.0)
    info = _lib.HarmonicInfo()
    st = c.lib.mfh_harmonic(c.h, prm, _lib.ptr(np.ascontiguousarray(om)), _lib.ptr(f), None, _lib.ptr(pv), len(pv), _lib.ptr(pout), _lib.ptr(fld),
                            _lib.ptr(its), _lib.ptr(res), info)
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.harmonic(om, f, density=H.DENSITY, damping=damping, rtol=RTOL, maxit=2)
    assert ei.value.code == _lib.ERR_NOT_CONVERGED and c.last_harmonic["info"]["freqsDone"] == expect
    c.close()
    print("full run iterations %s: freqsDone %d (expected %d)" % (list(full["iterations"]), info.freqsDone, expect))
    assert st == _lib.ERR_NOT_CONVERGED and info.freqsDone == expect
    done = slice(0, expect)
    assert np.array_equal(fld[done, 0] + 1j * fld[done, 1], full["u"][done]) and np.array_equal(its[done], full["iterations"][done])
    assert np.array_equal(pout[done, :, 0] + 1j * pout[done, :, 1], full["probes"][done])
    assert np.all(fld[expect:] == 7.0) and np.all(pout[expect:] == 7.0) and np.all(its[expect:] == -5) and np.all(res[expect:] == 7.0)


@pytest.mark.parametrize("storage", [None, 0], ids=["default-storage", "matrix_storage-0"])
def test_nothing_existing_moves(storage):
    """solve, apply_K, the exported triplets, modes and newmark (deterministic) give the same bits before and after a harmonic call."""
    key = (3, 2)
    opts = (("deterministic", 1),) + ((("matrix_storage", storage),) if storage is not None else ())
    c = _context(key, "multigrid", opts)
    f = H.load(key)
    w1 = float(H.natural_frequencies(key)[0])

    def snapshot():
        u = c.solve(f, rtol=1e-10)
        Kx = c.apply_K(f)
        c.assemble()
        A = c.export_scipy().tocsr()
        lam, X, _ = c.modes(3, density=H.DENSITY)
        nm = c.newmark(2.0 * np.pi / w1 / 20.0, 5, f=f, density=H.DENSITY, rtol=1e-10)
        return [u, Kx, A.indptr, A.indices, A.data, lam, X, nm["u"], nm["v"], nm["a"]]
    before = snapshot()
    r = _sweep(c, key, "rayleigh")
    assert _worst_error(r["u"], H.reference(key, "rayleigh")) <= BAR
    after = snapshot()
    c.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_mid_mesh():
    """37 905 unknowns, multigrid, Rayleigh case, omega in {omega_1 / 2, mid(omega_2, omega_3), mid(omega_5, omega_6)}."""
    key = U.MID
    om = tuple(H.sweep_omegas(key)[1:4])
    c = _context(key, "multigrid")
    r = _sweep(c, key, "rayleigh", omegas=om)
    c.close()
    err = _worst_error(r["u"], H.reference(key, "rayleigh", "real", om))
    print("mid mesh: error %.3e, iterations %s, true residuals %s, solve %.1f ms" % (err, list(r["iterations"]), list(r["true_residuals"]), r["info"]["solveMs"]))
    assert r["info"]["precondUsed"] == M.PRECOND_MULTIGRID
    assert err <= BAR and r["true_residuals"].max() <= 1e2 * RTOL
