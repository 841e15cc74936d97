"""The reference of the modal-superposition tests against itself (CPU only): the numpy formula of tests/modal_util.py on the dense eigenpairs of the
clamped pencil at harmonic_util.DENSITY against the complex direct solves of tests/harmonic_util.py, on the four small meshes, the three damping
cases, the complex load and the five sweep frequencies. What tests/test_gpu_modal.py takes from here: the full basis IS the direct solve (so the
formula is the right reference for the device), the static correction reduces the truncation error, and the rounding bound the device is held to
covers the float64 formula against its long-double twin."""
import numpy as np
import pytest
import scipy.sparse as sp

import harmonic_util as H
import modal_util as MU
import modes_util as U


def _name(key):
    return "%dD-P%d" % key


def _case(key, case):
    (aR, bR), eta = H.damping(key, case)
    return dict(aR=aR, bR=bR, eta=eta)


def _errors(key, case, m, corrected):
    lam, X = MU.clamped_basis(key)
    f = H.load(key, "complex")
    om = H.sweep_omegas(key)
    u, _ = MU.modal_response(lam[:m], X[:m], f, om, u_s=MU.static_solution(key) if corrected else None, **_case(key, case))
    ref = H.reference(key, case, "complex")
    return np.array([H.rel_l2(u[k], ref[k]) for k in range(len(om))])


@pytest.mark.parametrize("case", list(H.CASES))
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_full_basis_reproduces_the_direct_solve(key, case):
    lam, _ = MU.clamped_basis(key)
    err = _errors(key, case, len(lam), False)
    print("%s %s: full basis (%d modes) against the direct solve %s" % (_name(key), case, len(lam), err))
    assert err.max() <= 1e-10


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_static_correction_reproduces_the_static_solve(key):
    lam, X = MU.clamped_basis(key)
    f = H.load(key, "complex")
    us = MU.static_solution(key)
    for m in (4, 12, 24):
        u, _ = MU.modal_response(lam[:m], X[:m], f, [0.0], u_s=us)
        err = H.rel_l2(u[0], us)
        print("%s m %d: omega = 0 with the correction against the static solve %.3e" % (_name(key), m, err))
        assert err <= 1e-10


@pytest.mark.parametrize("case", list(H.CASES))
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_static_correction_reduces_the_truncation_error(key, case):
    om = H.sweep_omegas(key)
    e = {(m, c): _errors(key, case, m, c) for m in (12, 24) for c in (False, True)}
    for m in (12, 24):
        print("%s %s m %d: uncorrected %s corrected %s" % (_name(key), case, m, e[(m, False)], e[(m, True)]))
        assert np.all(e[(m, True)] < e[(m, False)])
    assert np.all(e[(24, True)][om > 0] < e[(12, True)][om > 0])


def test_modal_damping_is_a_direct_solve_with_its_damping_matrix():
    """Full basis, per-mode zeta: the formula equals the solve of (K - w^2 rho M + i w C) u = f with C = rho M Phi diag(2 zeta_j sqrt(lam_j)) Phi^T rho M."""
    key = (2, 1)
    lam, X = MU.clamped_basis(key)
    K, M = U.pencil(key)
    free = H.free_of(key)
    assert len(free) == 56 == len(lam)
    Kf, Mf = K[free][:, free].toarray(), H.DENSITY * M[free][:, free].toarray()
    Xf = X[:, free]
    zeta = 0.01 + 0.04 * np.random.default_rng(3).random(len(lam))
    Cd = Mf @ Xf.T @ np.diag(2.0 * zeta * np.sqrt(lam)) @ Xf @ Mf
    f = H.load(key, "complex")
    om = H.sweep_omegas(key)
    u, _ = MU.modal_response(lam, X, f, om, zeta=zeta)
    for k, w in enumerate(om):
        ref = np.linalg.solve(Kf - w * w * Mf + 1j * w * Cd, f[free])
        err = H.rel_l2(u[k][free], ref)
        print("zeta damping, omega %.4f: %.3e" % (w, err))
        assert err <= 1e-10


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_rounding_bound_covers_float64_against_long_double(key):
    """The bar of the device sweeps (modal_util.response_bound) is meant for this arithmetic: the float64 formula lies under it against the same
    formula in long double, for every case, truncation and correction the device tests run."""
    lam, X = MU.clamped_basis(key)
    f = H.load(key, "complex")
    om = H.sweep_omegas(key)
    n_free = len(H.free_of(key))
    worst = 0.0
    for case in H.CASES:
        for m in (4, 12, 24):
            for us in (None, MU.static_solution(key)):
                kw = dict(u_s=us, **_case(key, case))
                u64, _ = MU.modal_response(lam[:m], X[:m], f, om, **kw)
                ul, _ = MU.modal_response(lam[:m], X[:m], f, om, dtype=np.longdouble, **kw)
                bound = MU.response_bound(lam[:m], X[:m], f, om, n_free=n_free, rtol_static=0.0, **kw)
                diff = np.linalg.norm((u64 - ul).astype(np.complex128), axis=1)
                worst = max(worst, float((diff / bound).max()))
    print("%s: float64 against long double, worst ratio to the bound %.3e" % (_name(key), worst))
    assert worst <= 1.0
