"""The host arithmetic of the random-vibration layer (CPU only; docs/design/04_23_modal_random.md): psd_factor, modal_covariance, cqc_matrix and
resonance_grid against the numpy twins of tests/modal_random_util.py, and the method itself -- the quadratic form through the factor against the
sum over the frequencies of |u^(w_k)|^2 from tests/modal_util.py -- in numpy alone. The bars are 10 x the defect the float64 twin itself shows
(against the matrix for the factorisation, against its long-double twin for the covariance); they come from the twins, never from the library."""
import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import _lib

import harmonic_util as H
import modal_random_util as R
import modal_util as MU
import modes_util as U

EPS = R.EPS


def _name(key):
    return "%dD-P%d" % key


def _psd(n, rank, seed):
    rng = np.random.default_rng(seed)
    if rank == 0:
        return np.zeros((n, n))
    A = rng.standard_normal((n, rank)) * np.logspace(0, -3, rank)
    return A @ A.T


# ---------------------------------------------------------------- psd_factor
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 258])
def test_psd_factor_against_the_twin(n):
    """Ranks 0, 1, full and 4 = 2 nLoad nFreq (one load, two frequencies) where that is below n: rank and pivots equal the twin's, the defect
    |C - F F^T|_max and the truncation within 10 x the twin's."""
    for rank in sorted({0, 1, n} | ({4} if n > 4 else set())):
        C = _psd(n, rank, 100 * n + rank)
        Ft, pt, tt = R.psd_factor_twin(C)
        F, piv, trunc = M.psd_factor(C)
        d_twin, d_lib = np.abs(C - Ft @ Ft.T).max(), np.abs(C - F @ F.T).max()
        print("n %d rank %d: found %d (twin %d), defect %.3e (twin %.3e), truncation %.3e (twin %.3e)" % (n, rank, F.shape[1], Ft.shape[1], d_lib, d_twin, trunc, tt))
        assert F.shape == (n, Ft.shape[1]) and np.array_equal(piv, pt)
        assert F.shape[1] == rank if rank in (0, 1, 4) else F.shape[1] <= n
        assert d_lib <= 10.0 * d_twin
        assert abs(trunc - tt) <= 10.0 * d_twin and trunc >= 0.0
        for s_, p in enumerate(piv):          # the rows of the earlier pivots are exactly zero in the later columns
            assert np.all(F[p, s_ + 1:] == 0.0)
        # the remainder is what the truncation says it is
        assert abs(np.trace(C - F @ F.T) - trunc) <= 10.0 * n * max(d_twin, EPS * np.abs(C).max())


def test_psd_factor_tolerance_and_lower_triangle():
    C = _psd(33, 33, 7)
    F, piv, trunc = M.psd_factor(C, tol=1e-3 * C.diagonal().max())
    Ft, pt, tt = R.psd_factor_twin(C, tol=1e-3 * C.diagonal().max())
    assert 0 < F.shape[1] < 33 and np.array_equal(piv, pt) and trunc == tt
    rem = C - F @ F.T
    assert np.linalg.eigvalsh(rem).min() >= -1e-12 * C.diagonal().max() and rem.diagonal().max() <= 1e-3 * C.diagonal().max() * (1 + 1e-12)
    Cu = C.copy()
    Cu[np.triu_indices(33, 1)] = 123.0         # the upper triangle is not read
    F2, piv2, _ = M.psd_factor(Cu, tol=1e-3 * C.diagonal().max())
    assert np.array_equal(F2, F) and np.array_equal(piv2, piv)


def test_psd_factor_refusals():
    rng = np.random.default_rng(3)
    n = 24
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.linspace(0.1, 1.0, n)
    ev[5] = -1e-3
    C = (Q * ev) @ Q.T
    with pytest.raises(ValueError):
        R.psd_factor_twin(C)
    with pytest.raises(M.MeshFEMHipError) as ei:
        M.psd_factor(C)
    assert ei.value.code == _lib.ERR_INVALID
    for bad in (np.nan, np.inf):
        Cb = _psd(5, 5, 1)
        Cb[3, 1] = bad
        with pytest.raises(M.MeshFEMHipError) as ei:
            M.psd_factor(Cb)
        assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(M.MeshFEMHipError) as ei:
        M.psd_factor(np.eye(259))
    assert ei.value.code == _lib.ERR_INVALID


# ---------------------------------------------------------------- modal_covariance
LAM = np.array([1.0, 2.5, 2.6, 9.0, 30.0, 31.0, 120.0])
DAMPING = {"rayleigh": dict(aR=0.05, bR=0.004), "structural": dict(eta=0.03), "modal": dict(zeta=np.array([0.02, 0.01, 0.03, 0.02, 0.05, 0.02, 0.1]))}


def _spectrum(om, nl, seed):
    """A smooth Hermitian positive semi-definite S(w) with a complex cross term."""
    rng = np.random.default_rng(seed)
    A0, A1 = rng.standard_normal((2, nl, nl)) + 1j * rng.standard_normal((2, nl, nl))
    S = np.zeros((len(om), nl, nl), dtype=np.complex128)
    for k, w in enumerate(om):
        A = A0 + np.sin(0.3 * w) * A1
        Sk = A @ np.conj(A).T / (1.0 + 0.01 * w * w)
        S[k] = 0.5 * (Sk + np.conj(Sk).T)
    return S


def _lib_cov(lam, g, om, S, kw, correction, weights=None):
    return M.modal_covariance(lam, g, om, S, weights=weights, damping=(kw.get("aR", 0.0), kw.get("bR", 0.0)), loss_factor=kw.get("eta", 0.0),
                              modal_damping=kw.get("zeta"), correction=correction)


@pytest.mark.parametrize("correction", [False, True])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("case", list(DAMPING))
def test_covariance_against_the_long_double_twin(case, nl, correction):
    kw = DAMPING[case]
    rng = np.random.default_rng(5)
    g = rng.standard_normal((len(LAM), nl))
    om = np.unique(np.concatenate([np.linspace(0.0, 14.0, 41), np.sqrt(LAM) * (1 + 1e-3)]))
    S = _spectrum(om, nl, 11)
    ld = R.covariance_twin(LAM, g, om, S, correction=correction, dtype=np.longdouble, **kw)
    f64 = R.covariance_twin(LAM, g, om, S, correction=correction, **kw)
    lib = _lib_cov(LAM, g, om, S, kw, correction)
    nb = len(LAM) + (nl if correction else 0)
    assert lib.shape == ld.shape == (3, nb, nb)
    for p in range(3):
        twin = float(np.abs(f64[p] - ld[p]).max())
        err = float(np.abs(lib[p] - ld[p]).max())
        print("%s nLoad %d correction %d C^(%d): library %.3e, float64 twin %.3e (largest entry %.3e)" % (case, nl, correction, 2 * p, err, twin, np.abs(ld[p]).max()))
        assert err <= 10.0 * twin
        assert np.array_equal(lib[p], lib[p].T)
    # caller's weights: Simpson-like weights are taken as they are
    w = R.trapezoid_weights(om) * (1.0 + 0.1 * np.cos(np.arange(len(om))))
    ld = R.covariance_twin(LAM, g, om, S, weights=w, correction=correction, dtype=np.longdouble, **kw)
    f64 = R.covariance_twin(LAM, g, om, S, weights=w, correction=correction, **kw)
    lib = _lib_cov(LAM, g, om, S, kw, correction, weights=w)
    for p in range(3):
        assert np.abs(lib[p] - ld[p]).max() <= 10.0 * np.abs(f64[p] - ld[p]).max()


def test_covariance_is_reproducible():
    rng = np.random.default_rng(8)
    lam = np.sort(rng.uniform(1.0, 400.0, 200))
    g = rng.standard_normal((200, 2))
    om = np.linspace(0.0, 25.0, 300)
    S = _spectrum(om, 2, 4)
    a = M.modal_covariance(lam, g, om, S, modal_damping=0.02)
    assert np.array_equal(a, M.modal_covariance(lam, g, om, S, modal_damping=0.02))
    # 300 frequencies are five blocks of the host loop: the sum runs through them in grid order
    f64 = R.covariance_twin(lam, g, om, S, zeta=np.full(200, 0.02))
    ld = R.covariance_twin(lam, g, om, S, zeta=np.full(200, 0.02), dtype=np.longdouble)
    assert np.abs(a[0] - ld[0]).max() <= 10.0 * np.abs(f64[0] - ld[0]).max()


def test_fully_correlated_loads_are_one_summed_load():
    """S = s(w) [[1, 1], [1, 1]]: the two loads act as their sum. Both sides are library results; they differ by the rounding of the two-term sums
    g_a / d + g_b / d against (g_a + g_b) / d: the bar is 10 x the float64 twins' defects of the two problems."""
    kw = DAMPING["modal"]
    rng = np.random.default_rng(6)
    g = rng.standard_normal((len(LAM), 2))
    om = np.linspace(0.1, 14.0, 60)
    s = 1.0 / (1.0 + om)
    S2 = s[:, None, None] * np.ones((1, 2, 2))
    two = _lib_cov(LAM, g, om, S2, kw, False)
    one = _lib_cov(LAM, g.sum(axis=1), om, s, kw, False)
    for p in range(3):
        bar = 10.0 * (np.abs(R.covariance_twin(LAM, g, om, S2, **kw)[p] - R.covariance_twin(LAM, g, om, S2, dtype=np.longdouble, **kw)[p]).max() +
                      np.abs(R.covariance_twin(LAM, g.sum(axis=1), om, s, **kw)[p] - R.covariance_twin(LAM, g.sum(axis=1), om, s, dtype=np.longdouble, **kw)[p]).max() +
                      EPS * np.abs(one[p]).max())
        assert np.abs(two[p] - one[p]).max() <= bar


def test_covariance_refusals():
    g = np.ones(len(LAM))
    om = np.linspace(0.1, 5.0, 10)
    s = np.ones(10)
    kw = dict(modal_damping=0.02)

    def refused(code=_lib.ERR_INVALID, **over):
        args = dict(lam=LAM, g=g, omega=om, S=s)
        args.update(over)
        with pytest.raises(M.MeshFEMHipError) as ei:
            M.modal_covariance(args.pop("lam"), args.pop("g"), args.pop("omega"), args.pop("S"), **{**kw, **args})
        assert ei.value.code == code
    refused(omega=om[::-1].copy())                                        # descending
    refused(omega=np.concatenate([om[:5], om[4:9]]))                      # a repeated point
    refused(omega=om - 1.0)                                               # negative
    lam0 = LAM.copy()
    lam0[0] = 0.0
    refused(lam=lam0, omega=np.linspace(0.0, 5.0, 10))                    # omega = 0 with a zero lambda
    M.modal_covariance(lam0, g, om, s, **kw)                              # (a rigid mode alone is fine)
    refused(omega=np.array([0.5, 1.0, 2.0]), S=np.ones(3), modal_damping=None)          # undamped on an eigenfrequency: d_1 = 0
    S2 = _spectrum(om, 2, 1)
    bad = S2.copy()
    bad[3, 0, 1] += 1e-12 * np.abs(S2[3]).max()
    refused(g=np.ones((len(LAM), 2)), S=bad)                              # not Hermitian
    bad = S2.copy()
    bad[3, 1, 1] = -1e-300
    refused(g=np.ones((len(LAM), 2)), S=bad)                              # a negative diagonal
    for v in (np.nan, np.inf):
        b = s.copy()
        b[2] = v
        refused(S=b)
        b = g.copy()
        b[1] = v
        refused(g=b)
    refused(code=_lib.ERR_UNSUPPORTED, g=np.ones((len(LAM), 3)), S=_spectrum(om, 3, 2), correction=True)
    refused(omega=om[:1], S=s[:1])                                        # one point and no weights
    assert M.modal_covariance(LAM, g, om[:1], s[:1], weights=[2.0], **kw).shape == (3, len(LAM), len(LAM))


# ---------------------------------------------------------------- the method, numpy only
@pytest.mark.parametrize("corrected", [False, True])
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_factor_route_equals_the_sum_over_frequencies(key, corrected):
    """sigma_u^2 = sum_t (B F)_t^2 with C^(0) = F F^T from the twins against sum_k w_k S_k |u^(w_k)|^2 with u^ from modal_util.modal_response: the
    same quantity by two routes (24 modes, Rayleigh damping, 40 frequencies, one load). Bar: 1e-12 of the largest variance -- sums of at most
    (24 + 1) x 40 terms of one sign, a thousand roundings of headroom; the scratch check of the method gave 1e-15."""
    lam, X = MU.clamped_basis(key)
    lam, X = lam[:24], X[:24]
    f = np.asarray(H.load(key))
    (aR, bR), eta = H.damping(key, "rayleigh")
    w1 = np.sqrt(lam[0])
    om = np.linspace(0.2 * w1, 3.0 * w1, 40)
    S = 1.0 / (1.0 + (om / w1) ** 2)
    us = np.asarray(MU.static_solution(key, "real")).real if corrected else None
    u, _ = MU.modal_response(lam, X, f, om, aR=aR, bR=bR, eta=eta, u_s=us)
    wq = R.trapezoid_weights(om)
    direct = ((wq * S)[:, None] * np.abs(u) ** 2).sum(axis=0)
    g = X @ f
    B = X if not corrected else np.vstack([X, us - (g / lam) @ X])
    C0 = R.covariance_twin(lam, g, om, S, aR=aR, bR=bR, eta=eta, correction=corrected)[0]
    F, piv, trunc = R.psd_factor_twin(C0)
    route = ((B.T @ F) ** 2).sum(axis=1)
    err = np.abs(route - direct).max() / direct.max()
    print("%s corrected %d: rank %d of %d, truncation %.3e, factor route against the sum %.3e" % (_name(key), corrected, F.shape[1], C0.shape[0], trunc, err))
    assert F.shape[1] <= min(C0.shape[0], 2 * len(om))
    assert err <= 1e-12 + trunc * (np.linalg.norm(B, axis=0) ** 2).max() / direct.max()
    assert route.min() >= 0.0


# ---------------------------------------------------------------- cqc_matrix
def test_cqc_matrix():
    rng = np.random.default_rng(9)
    worst = np.inf
    for draw in range(200):
        m = 12
        lam = np.sort(rng.uniform(1.0, 100.0, m))
        lam[4] = lam[3] * (1.0 + 1e-3)                      # one close pair
        zeta = rng.uniform(0.005, 0.2, m)
        rho = M.cqc_matrix(lam, zeta)
        ref = R.cqc_twin(lam, zeta)
        assert np.array_equal(rho, rho.T) and np.all(rho.diagonal() == 1.0)
        assert np.abs(rho - ref.astype(np.float64)).max() <= 64 * EPS          # a dozen operations on numbers of order one
        worst = min(worst, np.linalg.eigvalsh(rho).min())
    print("cqc_matrix: smallest eigenvalue over 200 draws %.3e" % worst)
    assert worst >= 0.0
    assert M.cqc_matrix([4.0, 4.0, 9.0], 0.03)[0, 1] == 1.0                     # equal lambda, equal zeta
    far = M.cqc_matrix(100.0 ** np.arange(4), 0.02)                             # ratios of lambda >= 100
    assert np.abs(far - np.eye(4)).max() <= 2e-4
    for lam, zeta in (([1.0, -1.0], 0.02), ([1.0, 2.0], 0.0), ([1.0, np.nan], 0.02)):
        with pytest.raises(M.MeshFEMHipError) as ei:
            M.cqc_matrix(lam, zeta)
        assert ei.value.code == _lib.ERR_INVALID


# ---------------------------------------------------------------- resonance_grid
def test_resonance_grid_resolves_a_lightly_damped_mode():
    """One mode under white noise S0: the variance is pi S0 g^2 / (4 zeta w_n^3) (the integral over all frequencies; the band ends at 200 w_n, beyond
    which 4 zeta / (3 pi 200^3) = 1e-9 of it lies). The trapezoid rule on the grid approaches it at second order in per_halfpower."""
    wn, zeta, S0, g = 3.0, 0.02, 0.7, 1.3
    exact = np.pi * S0 * g * g / (4.0 * zeta * wn ** 3)
    errs = []
    for p in (2, 4, 8, 16):
        om = M.resonance_grid([wn * wn], zeta, (0.0, 200.0 * wn), per_halfpower=p, background=16)
        assert np.all(np.diff(om) > 0.0) and om[0] == 0.0 and om[-1] == 200.0 * wn
        var = M.modal_covariance([wn * wn], [g], om, np.full(om.size, S0), modal_damping=zeta)[0, 0, 0]
        errs.append(abs(var / exact - 1.0))
        print("per_halfpower %2d: %4d points, relative error %.3e" % (p, om.size, errs[-1]))
    assert errs[-1] <= 1e-4
    for a, b in zip(errs[:-1], errs[1:]):
        assert b <= a / 3.0
    # modes outside the band add nothing; several modes merge into one ascending grid
    om = M.resonance_grid([1.0, 4.0, 1e6], [0.01, 0.02, 0.01], (0.5, 10.0), per_halfpower=4)
    assert np.all(np.diff(om) > 0.0) and om[0] == 0.5 and om[-1] == 10.0
    assert np.diff(om)[np.searchsorted(om, 1.0) - 1] <= 2 * 0.01 / 4 * (1 + 1e-9)
