"""Shared helpers of the random-vibration tests (tests/test_modal_random_reference.py, tests/test_gpu_modal_sumsq.py, tests/test_gpu_modal_random.py,
tests/test_cpp_modal_random.py): numpy twins, in float64 and in np.longdouble, of

    H_k   = [ g_ja / d_j(w_k) ;  delta_ab / zK(w_k) ]                 (nb x nLoad; the second block only with the static correction)
    C^(p) = sum_k w_k w_k^p Re(H_k S_k H_k^H),  p = 0, 2, 4           (modal covariances of displacement, velocity, acceleration)
    sigma(i)^2 = phi_i^T C phi_i,                                      phi_i = row i of B = [Phi | r_1 | r_2]

of the diagonally pivoted Cholesky factorisation C = F F^T the library evaluates the form through, of the CQC correlation, and the rounding bound of
the device's sum of squares. None of it touches the library under test; d_j, zK and the modes are those of tests/modal_util.py."""
import numpy as np

import modal_util as MU

EPS = MU.EPS


def trapezoid_weights(om):
    om = np.asarray(om)
    w = np.zeros(len(om), dtype=om.dtype)
    w[1:] += 0.5 * (om[1:] - om[:-1])
    w[:-1] += 0.5 * (om[1:] - om[:-1])
    return w


def psd_factor_twin(C, tol=None):
    """(F [n, rank], piv, truncation): right-looking Cholesky with diagonal pivoting on a symmetric copy of the lower triangle, the operations of
    mfh_psd_factor one for one -- pivot = the first largest remaining diagonal, stop at <= tol (None: n eps max diag), column = W[:, p] / sqrt(W[p, p])
    with exact zeros on the rows chosen before, W -= column column^T (rounded product, rounded subtraction). Raises ValueError where a remaining
    diagonal is below -tol."""
    C = np.asarray(C, dtype=np.float64)
    n = C.shape[0]
    W = np.tril(C) + np.tril(C, -1).T
    if tol is None:
        tol = n * EPS * max(0.0, W.diagonal().max()) if n else 0.0
    chosen = np.zeros(n, dtype=bool)
    cols, piv = [], []
    while True:
        d = np.where(chosen, -np.inf, W.diagonal())
        if np.any(~chosen & (W.diagonal() < -tol)):
            raise ValueError("not positive semi-definite")
        if chosen.all():
            break
        p = int(np.argmax(d))
        if not d[p] > tol:
            break
        l = np.sqrt(W[p, p])
        col = np.where(chosen, 0.0, W[:, p] / l)
        col[p] = l
        W = W - np.outer(col, col)
        chosen[p] = True
        cols.append(col)
        piv.append(p)
    F = np.array(cols).T.reshape(n, len(cols))
    trunc = 0.0
    for i in range(n):
        if not chosen[i]:
            trunc = trunc + max(W[i, i], 0.0)
    return F, np.array(piv, dtype=np.int32), trunc


def transfer(lam, g, w, aR=0.0, bR=0.0, eta=0.0, zeta=None, correction=False, dtype=np.float64):
    """H(w), [nb, nLoad] complex: g_ja / d_j on the modes, then (with correction) the identity / zK on the nLoad correction columns. The reciprocals
    are formed as conj(d) / |d|^2 and multiplied, as the library does."""
    ct = np.clongdouble if dtype == np.longdouble else np.complex128
    g = np.asarray(g, dtype=dtype).reshape(len(lam), -1)
    d = MU.denominators(lam, w, aR, bR, eta, zeta, dtype)
    di = np.conj(d) / (d.real * d.real + d.imag * d.imag)
    H = g.astype(ct) * di[:, None]
    if correction:
        zK = ct(1 + 1j * ct(dtype(eta) + dtype(w) * dtype(bR)))
        iz = np.conj(zK) / (zK.real * zK.real + zK.imag * zK.imag)
        H = np.concatenate([H, np.eye(g.shape[1], dtype=ct) * iz])
    return H


def covariance_twin(lam, g, om, S, weights=None, aR=0.0, bR=0.0, eta=0.0, zeta=None, correction=False, dtype=np.float64):
    """[3, nb, nb]: C^(0), C^(2), C^(4), the sum over k in grid order in the precision of dtype."""
    ct = np.clongdouble if dtype == np.longdouble else np.complex128
    om = np.asarray(om, dtype=dtype)
    w = trapezoid_weights(om) if weights is None else np.asarray(weights, dtype=dtype)
    S = np.asarray(S).astype(ct)
    if S.ndim == 1:
        S = S.reshape(-1, 1, 1)
    out = None
    for k in range(len(om)):
        H = transfer(lam, g, om[k], aR, bR, eta, zeta, correction, dtype)
        M = ((H @ S[k]) @ np.conj(H).T).real
        if out is None:
            out = np.zeros((3,) + M.shape, dtype=dtype)
        w2 = om[k] * om[k]
        out[0] += w[k] * M
        out[1] += (w[k] * w2) * M
        out[2] += ((w[k] * w2) * w2) * M
    return out


def cqc_twin(lam, zeta, dtype=np.longdouble):
    """rho_jk = 8 sqrt(z_j z_k) (z_j + r z_k) r^(3/2) / ((1 - r^2)^2 + 4 z_j z_k r (1 + r^2) + 4 (z_j^2 + z_k^2) r^2), r = w_k / w_j, as it stands."""
    w = np.sqrt(np.asarray(lam, dtype=dtype))
    z = np.broadcast_to(np.asarray(zeta, dtype=dtype), w.shape)
    r = w[None, :] / w[:, None]
    zj, zk = z[:, None], z[None, :]
    return 8 * np.sqrt(zj * zk) * (zj + r * zk) * r ** dtype(1.5) / ((1 - r * r) ** 2 + 4 * zj * zk * r * (1 + r * r) + 4 * (zj * zj + zk * zk) * r * r)


def sumsq_prefixes(B, F, ranks):
    """{r: (reference [n] in long double, bound [n], reference of the root, bound of the root)} of v = sum_{t < r} (sum_j B[j] F[j, t])^2 for the leading r columns of F, the long-double product
    B^T F taken once. The bound on the device's v, s_t the fma chain over the nb columns and v the chain fma(s_t, s_t, .) over t:
        delta_t = (nb + 1) eps sum_j |B_j| |F_jt|,
        |v - v_exact| <= sum_t (2 |y_t| delta_t + delta_t^2) + (r + 2) eps sum_t y_t^2,
    and for the root one more rounding: |sqrt(v~) - sqrt(v)| <= min(|v~ - v| / sqrt(v), sqrt|v~ - v|), plus 2 eps sqrt(v)."""
    B, F = np.asarray(B, dtype=np.float64), np.asarray(F, dtype=np.float64)
    nb = F.shape[0]
    y = np.ascontiguousarray(B.T.astype(np.longdouble)) @ F.astype(np.longdouble)
    ya = np.abs(y).astype(np.float64)
    delta = (nb + 1) * EPS * (np.abs(B).T @ np.abs(F))
    tiny = np.finfo(float).tiny
    out = {}
    for r in ranks:
        v = (y[:, :r] * y[:, :r]).sum(axis=1)
        vf = v.astype(np.float64)
        bv = ((2 * ya[:, :r] * delta[:, :r] + delta[:, :r] ** 2).sum(axis=1) + (r + 2) * EPS * vf) * (1 + 8 * EPS) + tiny
        sv = np.sqrt(vf)
        b = np.where(sv > 0, np.minimum(bv / np.where(sv > 0, sv, 1.0), np.sqrt(bv)), np.sqrt(bv))
        out[r] = (v, bv, np.sqrt(v), b * (1 + 8 * EPS) + 2 * EPS * sv + tiny)
    return out


def rms_reference(X, cov, dtype=np.longdouble):
    """sqrt(phi_i^T C phi_i) for the rows phi_i of X^T ([nb, n] rows = columns of the basis): [n], the form evaluated as it stands in dtype."""
    Xd = np.asarray(X, dtype=dtype)
    v = np.einsum("ji,jk,ki->i", Xd, np.asarray(cov, dtype=dtype), Xd)
    return np.sqrt(np.maximum(v, 0))
