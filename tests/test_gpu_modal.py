"""Modal superposition on the device (mfh_modal_set_basis, mfh_modal_coordinates, mfh_modal_harmonic) against the numpy formula of
tests/modal_util.py evaluated on the SAME modes (scipy's dense eigenpairs of the pencil of tests/modes_util.py at harmonic_util.DENSITY), on the
four small meshes; against the complex direct solves of tests/harmonic_util.py with a full basis; against Context.solve / Context.harmonic on
the same context where the statement is about them. The bars are rounding bounds of the sums involved (modal_util.response_bound, coords_bound,
gram_bound; the test of each states what it adds), worked out from the reference data, never from the device's output.
tests/test_modal_reference.py shows on the CPU that the formula is the right reference and that the bounds are meant for this arithmetic."""
import numpy as np
import pytest
import scipy.sparse as sp

import meshfem_amd as M
from meshfem_amd import _lib

import harmonic_util as H
import modal_util as MU
import modes_util as U

pytestmark = pytest.mark.gpu

EPS = U.EPS
RTOL = MU.RTOL_STATIC
MAXIT = 20000
PRECONDS = {"jacobi": M.PRECOND_BLOCK_JACOBI, "two-level": M.PRECOND_TWO_LEVEL, "multigrid": M.PRECOND_MULTIGRID}


def _name(key):
    return key if isinstance(key, str) else "%dD-P%d" % key


def _context(key, precond="multigrid", options=(), clamped=True):
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


def _basis(key, m):
    lam, X = MU.clamped_basis(key)
    return lam[:m], X[:m]


def _case(key, case, clamped=True):
    (aR, bR), eta = H.damping(key, case, clamped)
    return dict(aR=aR, bR=bR, eta=eta)


def _sweep(c, key, case, kind="complex", omegas=None, clamped=True, **kw):
    damping, eta = H.damping(key, case, clamped)
    args = dict(damping=damping, loss_factor=eta, rtol=RTOL, maxit=MAXIT)
    args.update(kw)
    return c.modal_harmonic(H.sweep_omegas(key) if omegas is None else omegas, H.load(key, kind, clamped), **args)


def _norms(a):
    return np.linalg.norm(a, axis=1)


def _rho_m(key):
    return H.DENSITY * U.pencil(key)[1]


# ---------------------------------------------------------------- the basis
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_set_modal_basis(key):
    """orthoDefect of scipy's modes: at most the rounding bound of the Gram sums, (n + 1) eps sum |phi_i| |rho M phi_j| (largest entry); a column
    scaled by s reports |s^2 - 1| within the bound of the scaled set. (scipy's own defect, printed, is a tenth of the bound or less.)"""
    lam, X = _basis(key, 64)
    m = len(lam)
    rM = _rho_m(key)
    n_free = len(H.free_of(key))
    c = _context(key)
    for s in (1.0, 1.5):
        Xs = X.copy()
        Xs[3] *= s
        MX = (rM @ Xs.T).T
        host = np.abs(Xs @ MX.T - np.eye(m)).max()
        bound = MU.gram_bound(Xs, MX, n_free).max()
        info = c.set_modal_basis(lam, Xs, density=H.DENSITY)
        print("%s scale %.1f: %d modes, orthoDefect %.3e, host %.3e, bound %.3e, %.0f bytes" % (_name(key), s, m, info["orthoDefect"], host, bound, info["deviceBytes"]))
        assert info["nModes"] == m and info["ld"] % 32 == 0 and info["ld"] >= X.shape[1]
        if s == 1.0:
            assert info["orthoDefect"] <= bound
        else:
            assert abs(info["orthoDefect"] - abs(s * s - 1.0)) <= bound
    c.close()


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_modal_coordinates(key):
    """Of the basis's own modes: the identity; of random fields (non-zero on the clamp too): X (rho M u) from scipy. Both within the bound of the sums.
    Nine fields: more than one batch of the mass product."""
    lam, X = _basis(key, 24)
    m = len(lam)
    rM = _rho_m(key)
    n_free = len(H.free_of(key))
    c = _context(key, options=(("deterministic", 1),))         # (every call assembles the mass values again: the same bits only from the ordered sums)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    q = c.modal_coordinates(X)
    MX = (rM @ X.T).T
    bound = MU.gram_bound(X, MX, n_free)
    assert q.shape == (m, m)
    assert np.all(np.abs(q.T - np.eye(m)) <= bound)
    u = np.random.default_rng(2).standard_normal((9, X.shape[1]))
    Mu = (rM @ u.T).T
    q2 = c.modal_coordinates(u)
    ref = (X @ Mu.T).T
    b2 = MU.gram_bound(X, Mu, X.shape[1]).T
    print("%s: own modes %.3e of the bound, random fields %.3e" % (_name(key), (np.abs(q.T - np.eye(m)) / bound).max(), (np.abs(q2 - ref) / b2).max()))
    assert q2.shape == (9, m) and np.all(np.abs(q2 - ref) <= b2)
    assert np.array_equal(c.modal_coordinates(u[0]), q2[0])
    c.close()


# ---------------------------------------------------------------- the sweep against the formula on the same modes
@pytest.mark.parametrize("case", list(H.CASES))
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_against_the_formula(key, case):
    """m in {4, 12, 24}, static correction on and off, real and complex load, the five sweep frequencies: fields within response_bound (the Gram sums
    of g, the formation of q and the fma chain of the expansion; corrected runs add 10 rtol ||u_s|| / |zK| for the static solve at rtol 1e-12),
    modal coordinates within coords_bound."""
    om = H.sweep_omegas(key)
    n_free = len(H.free_of(key))
    kw = _case(key, case)
    c = _context(key)
    for m in (4, 12, 24):
        lam, X = _basis(key, m)
        c.set_modal_basis(lam, X, density=H.DENSITY)
        for kind in ("real", "complex"):
            f = H.load(key, kind)
            for corrected in (False, True):
                us = MU.static_solution(key, kind) if corrected else None
                r = _sweep(c, key, case, kind, static_correction=corrected)
                ref, q = MU.modal_response(lam, X, f, om, u_s=us, **kw)
                bar = MU.response_bound(lam, X, f, om, u_s=us, n_free=n_free, **kw)
                qbar = MU.coords_bound(lam, X, f, om, n_free=n_free, **kw)
                err = _norms(r["u"] - ref)
                print("%s %s m %d %s corrected %d: error / bar %s, coordinates %.3e of their bar, note '%s'" %
                      (_name(key), case, m, kind, corrected, err / bar, (np.abs(r["modal_coords"] - q) / qbar).max(), r["info"]["note"]))
                assert np.all(err <= bar)
                assert np.all(np.abs(r["modal_coords"] - q) <= qbar)
                assert np.all(r["u"][:, U.clamp_vars(key)] == 0.0)
                assert np.all(r["true_residuals"] == -1.0)
                assert r["info"]["planesPerPass"] == MU.NP_DEFAULT
                assert r["info"]["staticSolves"] == (0 if not corrected else (2 if kind == "complex" else 1))
    c.close()


@pytest.mark.parametrize("case", list(H.CASES))
def test_full_basis_against_the_direct_solve(case):
    """All 56 modes of the 2D linear mesh: the device sweep against harmonic_util.reference, within 10 x the defect the CPU formula itself shows
    against that direct solve (never below 1e-10)."""
    key = (2, 1)
    lam, X = MU.clamped_basis(key)
    assert len(lam) == 56
    om = H.sweep_omegas(key)
    f = H.load(key, "complex")
    ref = H.reference(key, case, "complex")
    cpu, _ = MU.modal_response(lam, X, f, om, **_case(key, case))
    bar = max(10.0 * max(H.rel_l2(cpu[k], ref[k]) for k in range(len(om))), 1e-10)
    c = _context(key)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    r = _sweep(c, key, case, static_correction=False)
    c.close()
    err = max(H.rel_l2(r["u"][k], ref[k]) for k in range(len(om)))
    print("2D-P1 %s full basis: %.3e (bar %.3e)" % (case, err, bar))
    assert err <= bar


# ---------------------------------------------------------------- individual properties
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_static_limit_is_context_solve(key):
    """omega = 0, no damping, real load, correction on: u^ = sum phi_j q_j + (u_s - sum phi_j q_j) with u_s the bits of Context.solve at the same
    rtol -- up to the two fma chains: 8 (m + 2) eps sum_j |q_j| ||phi_j||_2."""
    m = 12
    lam, X = _basis(key, m)
    f = H.load(key)
    c = _context(key, options=(("deterministic", 1),))
    u = c.solve(f, rtol=RTOL, maxit=MAXIT)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    r = c.modal_harmonic([0.0], f, rtol=RTOL, maxit=MAXIT)
    c.close()
    q = (X @ f) / lam
    bar = 8 * (m + 2) * EPS * (np.abs(q) @ _norms(X))
    err = np.linalg.norm(r["u"][0].real - u)
    print("%s: omega = 0 against solve %.3e (bar %.3e)" % (_name(key), err, bar))
    assert err <= bar and np.all(r["u"].imag == 0.0)


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_probes_are_the_field_entries(key):
    lam, X = _basis(key, 24)
    free = H.free_of(key)
    pv = np.array([free[0], free[len(free) // 2], free[-1], free[0], U.clamp_vars(key)[0]], dtype=np.int64)
    c = _context(key, options=(("deterministic", 1),))         # (two calls make two static solves: the same bits only from the ordered sums)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    om = np.concatenate([H.sweep_omegas(key), np.linspace(0.1, 2.0, 40) * float(H.natural_frequencies(key)[0])])     # 45 frequencies: 90 planes, six passes
    a = _sweep(c, key, "rayleigh", omegas=om, probes=pv)
    b = _sweep(c, key, "rayleigh", omegas=om, probes=pv, fields=False)
    c.close()
    assert a["probes"].shape == (len(om), len(pv)) and b["u"] is None
    assert np.array_equal(a["probes"], a["u"][:, pv])
    assert np.array_equal(a["probes"], b["probes"])


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_real_load_without_damping_stays_real(key):
    lam, X = _basis(key, 12)
    c = _context(key)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    for corrected in (False, True):
        r = _sweep(c, key, "undamped", "real", static_correction=corrected)
        assert np.all(r["u"].imag == 0.0) and np.all(r["modal_coords"].imag == 0.0)
    c.close()


@pytest.mark.parametrize("two_pass,cap", [(0, 2048), (1, 2048), (0, 1)], ids=["one-pass", "two-pass", "one-workgroup"])
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_true_residuals(key, two_pass, cap):
    """residual_stride 0 and 2: ||f^ - Z u^|| / ||f^|| of the device's own u^ formed with the scipy pencil; the two differ by at most the norm of the
    product's rounding bound 4 L eps (|zK| |K| + |zM| |M|) |u^| (tests/test_gpu_harmonic.py) over ||f^||. Skipped entries are -1. one-workgroup:
    option dyn_grid_cap 1, so that the lanes of the norm kernel and of the mass product loop over the rows."""
    lam, X = _basis(key, 12)
    K, Mm = U.pencil(key)
    free = H.free_of(key)
    f = H.load(key, "complex")
    L = int(np.diff(K.indptr).max())
    om = H.sweep_omegas(key)
    c = _context(key, options=(("harmonic_two_pass", two_pass), ("dyn_grid_cap", cap)))
    c.set_modal_basis(lam, X, density=H.DENSITY)
    for stride in (0, 2):
        r = _sweep(c, key, "rayleigh", residual_stride=stride)
        worst = 0.0
        for k, w in enumerate(om):
            if k % max(stride, 1):
                assert r["true_residuals"][k] == -1.0
                continue
            zK, zM = H.coefficients(key, "rayleigh", float(w))
            u = r["u"][k]
            res = (f - (zK * (K @ u) + zM * (Mm @ u)))[free]
            want = np.linalg.norm(res) / np.linalg.norm(f)
            tol = np.linalg.norm((4 * L * EPS * (abs(zK) * (abs(K) @ np.abs(u)) + abs(zM) * (abs(Mm) @ np.abs(u))))[free]) / np.linalg.norm(f)
            worst = max(worst, abs(r["true_residuals"][k] - want) / tol)
            assert abs(r["true_residuals"][k] - want) <= tol
        done = r["true_residuals"][r["true_residuals"] >= 0]
        assert r["info"]["worstTrueResidual"] == done.max()
        print("%s two-pass %d stride %d: residuals %s, worst difference / tolerance %.3e, note '%s'" % (_name(key), two_pass, stride, r["true_residuals"], worst, r["info"]["note"]))
    c.close()


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_modal_damping(key):
    """Per-mode damping ratios (with Rayleigh damping on top, corrected and not) against the formula."""
    m = 12
    lam, X = _basis(key, m)
    zeta = 0.01 + 0.04 * np.random.default_rng(3).random(m)
    om = H.sweep_omegas(key)
    f = H.load(key, "complex")
    n_free = len(H.free_of(key))
    kw = dict(zeta=zeta, **_case(key, "rayleigh"))
    c = _context(key)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    for corrected in (False, True):
        us = MU.static_solution(key) if corrected else None
        r = _sweep(c, key, "rayleigh", modal_damping=zeta, static_correction=corrected)
        ref, q = MU.modal_response(lam, X, f, om, u_s=us, **kw)
        bar = MU.response_bound(lam, X, f, om, u_s=us, n_free=n_free, **kw)
        err = _norms(r["u"] - ref)
        print("%s zeta corrected %d: error / bar %s" % (_name(key), corrected, err / bar))
        assert np.all(err <= bar)
        assert np.all(np.abs(r["modal_coords"] - q) <= MU.coords_bound(lam, X, f, om, n_free=n_free, **kw))
    one = _sweep(c, key, "rayleigh", modal_damping=0.02, static_correction=False)          # a scalar: the same ratio for every mode
    ref1, _ = MU.modal_response(lam, X, f, om, **dict(kw, zeta=np.full(m, 0.02)))
    assert np.all(_norms(one["u"] - ref1) <= MU.response_bound(lam, X, f, om, n_free=n_free, **dict(kw, zeta=np.full(m, 0.02))))
    c.close()


# ---------------------------------------------------------------- free body
def test_free_body():
    """No fixed variables: the three M-orthonormalised rigid modes (lambda = 0) and 12 elastic modes; omega between the first two distinct free
    frequencies against the formula. omega = 0 and the static correction are refused."""
    key = (2, 2)
    K, Mm = U.pencil(key)
    rM = H.DENSITY * Mm
    lam_all, X_all = U.free_truth(key, nev_max=15)[:2]
    Z = U.m_orthonormalise(U.rigid_modes(U.fem_mesh(key).node_pos), rM)
    lam = np.concatenate([np.zeros(3), lam_all[3:15] / H.DENSITY])
    X = np.concatenate([Z.T, X_all[:, 3:15].T / np.sqrt(H.DENSITY)])
    w = H.natural_frequencies(key, clamped=False)
    second = w[np.nonzero(w > w[0] * (1 + 1e-6))[0][0]]
    om = (0.5 * (float(w[0]) + float(second)),)
    f = H.load(key, "complex", clamped=False)
    c = _context(key, clamped=False)
    info = c.set_modal_basis(lam, X, density=H.DENSITY)
    assert info["orthoDefect"] <= 1e-10
    for case in ("undamped", "rayleigh"):
        kw = _case(key, case, clamped=False)
        r = _sweep(c, key, case, omegas=om, clamped=False, static_correction=False)
        ref, q = MU.modal_response(lam, X, f, om, **kw)
        bar = MU.response_bound(lam, X, f, om, **kw)
        err = _norms(r["u"] - ref)
        print("2D-P2 free %s: error / bar %s" % (case, err / bar))
        assert np.all(err <= bar)
    with pytest.raises(M.MeshFEMHipError) as ei:
        _sweep(c, key, "undamped", omegas=(0.0,), clamped=False, static_correction=False)
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(M.MeshFEMHipError) as ei:
        _sweep(c, key, "undamped", omegas=om, clamped=False, static_correction=True)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    c.close()


# ---------------------------------------------------------------- refusals, state
def _code(call):
    with pytest.raises(M.MeshFEMHipError) as ei:
        call()
    return ei.value.code


def test_refusals():
    key = (3, 1)
    lam, X = _basis(key, 8)
    f = H.load(key)
    om = H.sweep_omegas(key)
    V, T, deg, _ = U.mesh_arrays(key)
    c = _context(key)
    assert c.modal_basis_state() == (0, False)
    assert _code(lambda: c.modal_harmonic(om, f, static_correction=False)) == _lib.ERR_STATE            # no basis
    assert _code(lambda: c.modal_coordinates(f)) == _lib.ERR_STATE
    set_ = lambda: c.set_modal_basis(lam, X, density=H.DENSITY)
    sweep = lambda **kw: c.modal_harmonic(om, f, static_correction=False, **kw)
    set_()
    first = sweep()
    assert c.modal_basis_state() == (8, True)
    c.fix_variables([int(H.free_of(key)[-1])])
    assert _code(sweep) == _lib.ERR_STATE and c.modal_basis_state() == (8, False)
    c.clear_fixed()
    assert _code(lambda: c.modal_harmonic(om[1:], f, static_correction=False)) == _lib.ERR_STATE and c.modal_basis_state() == (8, False)
    c.fix_variables(U.clamp_vars(key)[::-1].copy())                                                     # the same set again (in another order): the basis serves
    assert c.modal_basis_state() == (8, True) and np.array_equal(sweep()["u"], first["u"])
    c.set_density(np.full(c.n_elem, 2.0))
    assert _code(sweep) == _lib.ERR_STATE
    c.set_density(None)
    set_()
    sweep()
    c.mesh_update_vertices(np.ascontiguousarray(V) * 1.0)
    assert _code(sweep) == _lib.ERR_STATE and _code(lambda: c.modal_coordinates(f)) == _lib.ERR_STATE
    set_()
    c.material_isotropic(2.0 * U.E_MOD, U.NU)
    assert _code(sweep) == _lib.ERR_STATE
    c.material_isotropic(U.E_MOD, U.NU)
    set_()
    assert _code(lambda: sweep(residual_stride=0, modal_damping=0.01)) == _lib.ERR_INVALID              # a residual against per-mode damping
    for bad in (dict(rtol=2.0), dict(maxit=0), dict(damping=(-1.0, 0.0)), dict(loss_factor=-0.1), dict(modal_damping=-0.01), dict(probes=[c.bs * c.n_dof]),
                dict(residual_stride=-1)):
        assert _code(lambda: sweep(**bad)) == _lib.ERR_INVALID, bad
    assert _code(lambda: c.modal_harmonic([-1.0], f, static_correction=False)) == _lib.ERR_INVALID
    lam4 = lam.copy()
    lam4[2] = 4.0
    c.set_modal_basis(lam4, X, density=H.DENSITY)
    assert _code(lambda: c.modal_harmonic([2.0], f, static_correction=False)) == _lib.ERR_INVALID        # undamped on an eigenfrequency: d_j = 0 exactly
    set_()
    assert _code(lambda: c.set_modal_basis(lam, X, density=0.0)) == _lib.ERR_INVALID
    assert _code(lambda: c.set_modal_basis(-lam, X, density=1.0)) == _lib.ERR_INVALID
    Xn = X.copy()
    Xn[2, 5] = np.nan
    assert _code(lambda: c.set_modal_basis(lam, Xn, density=1.0)) == _lib.ERR_INVALID
    assert c.lib.mfh_modal_set_basis(c.h, 257, _lib.ptr(np.ascontiguousarray(lam)), _lib.ptr(np.ascontiguousarray(X)), 1.0, None) == _lib.ERR_INVALID
    assert c.lib.mfh_modal_set_basis(c.h, -1, _lib.ptr(np.ascontiguousarray(lam)), _lib.ptr(np.ascontiguousarray(X)), 1.0, None) == _lib.ERR_INVALID
    assert _code(lambda: c.modal_harmonic(om, f, rtol=1e-12, maxit=1)) == _lib.ERR_NOT_CONVERGED         # the static solve of the correction
    assert not c.last_modal_harmonic["u"].any() and np.all(c.last_modal_harmonic["true_residuals"] == -1.0)     # ... nothing written
    sweep()                                                                                              # the refused calls left the basis in place
    # nModes = 0 releases the device memory
    info = set_()
    live = M.device_arena_stats(0)["live_bytes"]
    c.set_modal_basis(None, None)
    assert M.device_arena_stats(0)["live_bytes"] == live - int(info["deviceBytes"])
    assert _code(sweep) == _lib.ERR_STATE
    c.close()


@pytest.mark.parametrize("storage", [None, 0], ids=["default-storage", "matrix_storage-0"])
def test_nothing_existing_moves(storage):
    """solve, apply_K, modes, harmonic and newmark (deterministic) give the same bits before a modal sweep, after setting the basis, and after the
    sweep (with static correction and residuals: every path of the call)."""
    key = (3, 2)
    opts = (("deterministic", 1),) + ((("matrix_storage", storage),) if storage is not None else ())
    c = _context(key, "multigrid", opts)
    f = H.load(key)
    w1 = float(H.natural_frequencies(key)[0])
    damping, eta = H.damping(key, "rayleigh")

    def snapshot():
        u = c.solve(f, rtol=1e-10)
        Kx = c.apply_K(f)
        lam, X, _ = c.modes(3, density=H.DENSITY)
        hr = c.harmonic([0.5 * w1], f, density=H.DENSITY, damping=damping, rtol=1e-10)
        nm = c.newmark(2.0 * np.pi / w1 / 20.0, 5, f=f, density=H.DENSITY, rtol=1e-10)
        return [u, Kx, lam, X, hr["u"], hr["iterations"], nm["u"], nm["v"], nm["a"]]
    before = snapshot()
    lam, X = _basis(key, 12)
    c.set_modal_basis(lam, X, density=H.DENSITY)
    between = snapshot()
    r = _sweep(c, key, "rayleigh", residual_stride=0)
    assert r["info"]["staticSolves"] == 2
    after = snapshot()
    r2 = _sweep(c, key, "rayleigh", residual_stride=0)
    c.close()
    for a, b, d in zip(before, between, after):
        assert np.array_equal(a, b) and np.array_equal(a, d)
    assert np.array_equal(r["u"], r2["u"]) and np.array_equal(r["true_residuals"], r2["true_residuals"])


# ---------------------------------------------------------------- end to end
def test_mid_mesh_end_to_end():
    """37 905 unknowns, multigrid, clamped: modal_basis(30), a Rayleigh sweep of 200 frequencies over [0.2 omega_1, 0.8 omega_30] with static
    correction and a true residual at every 50th frequency, checked against the scipy-pencil residual of the returned field (the tolerance of
    test_true_residuals). At omega_1 / 2 the field against Context.harmonic on the same context: truncation error nobody has measured, so the
    difference is printed and only has to be finite and below the uncorrected run's (what tests/test_modal_reference.py establishes on the small
    meshes)."""
    key = U.MID
    c = _context(key)
    lam, X, info = c.modal_basis(30, density=H.DENSITY, batch=12, rtol=1e-6, maxit=3000)
    assert len(lam) == 30 and info["modal_basis"]["nModes"] == 30
    print("mid mesh: modes_many %.0f ms, set_modal_basis %.1f ms, orthoDefect %.3e" % (info["solve_ms"], info["modal_basis"]["setupMs"], info["modal_basis"]["orthoDefect"]))
    assert info["modal_basis"]["orthoDefect"] <= 1e-6
    w = np.sqrt(lam)
    om = np.linspace(0.2 * w[0], 0.8 * w[29], 200)
    f = H.load(key, "real")
    aR, bR = 0.1 * w[0], 0.02 / w[0]
    pv = H.free_of(key)[[0, -1]]
    r = c.modal_harmonic(om, f, damping=(aR, bR), residual_stride=50, rtol=1e-10, maxit=MAXIT, probes=pv)
    K, Mm = U.pencil(key)
    free = H.free_of(key)
    L = int(np.diff(K.indptr).max())
    fn = np.linalg.norm(f)
    for k in range(200):
        if k % 50:
            assert r["true_residuals"][k] == -1.0
            continue
        zK, zM = complex(1.0, om[k] * bR), H.DENSITY * complex(-om[k] ** 2, om[k] * aR)
        u = r["u"][k]
        want = np.linalg.norm((f - (zK * (K @ u) + zM * (Mm @ u)))[free]) / fn
        tol = np.linalg.norm((4 * L * EPS * (abs(zK) * (abs(K) @ np.abs(u)) + abs(zM) * (abs(Mm) @ np.abs(u))))[free]) / fn
        print("mid mesh: omega %.4f true residual %.6e (scipy %.6e, tolerance %.1e)" % (om[k], r["true_residuals"][k], want, tol))
        assert abs(r["true_residuals"][k] - want) <= tol
    assert np.array_equal(r["probes"], r["u"][:, pv])
    print("mid mesh: sweep of 200 frequencies %.1f ms in %d groups (setup %.1f ms, %d static iterations)" %
          (r["info"]["solveMs"], r["info"]["groups"], r["info"]["setupMs"], r["info"]["staticIterations"]))
    w0 = [0.5 * w[0]]
    full = c.harmonic(w0, f, density=H.DENSITY, damping=(aR, bR), rtol=1e-10, maxit=MAXIT)["u"][0]
    cor = c.modal_harmonic(w0, f, damping=(aR, bR), rtol=1e-10, maxit=MAXIT)["u"][0]
    unc = c.modal_harmonic(w0, f, damping=(aR, bR), static_correction=False)["u"][0]
    c.close()
    d_cor, d_unc = H.rel_l2(cor, full), H.rel_l2(unc, full)
    print("mid mesh: omega_1 / 2 against harmonic: corrected %.3e, uncorrected %.3e" % (d_cor, d_unc))
    assert np.isfinite(d_cor) and d_cor < d_unc
