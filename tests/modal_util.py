"""Shared helpers of the modal-superposition tests (tests/test_modal_reference.py, tests/test_gpu_modal.py, tests/test_gpu_modal_expand.py,
tests/test_cpp_modal.py): the mode bases from scipy's dense eigh of the pencil of tests/modes_util.py at harmonic_util.DENSITY, the numpy form of

    u^(w) = sum_j phi_j q_j(w) [+ r_s / zK(w)],   q_j = (phi_j^T f^) / d_j,
    d_j = lam_j (1 + i (eta + w bR)) - w^2 + i w aR + 2 i zeta_j sqrt(lam_j) w,   zK = 1 + i (eta + w bR),
    r_s = u_s - sum_j phi_j (phi_j^T f^) / lam_j,   K u_s = f^

in float64 and in np.longdouble, and the rounding bounds the device results are held to. None of it touches the library under test. Every reference
is computed once per process (functools.lru_cache) and handed out read-only."""
import functools

import numpy as np
import scipy.linalg

import harmonic_util as H
import modes_util as U

EPS = U.EPS
NP_DEFAULT = 32          # planes per pass of k_modal_expand (mfh_modal_harmonic_info::planesPerPass; tests/test_gpu_modal.py checks it is this)
RTOL_STATIC = 1e-12      # the static solves of the corrected runs


@functools.lru_cache(maxsize=None)
def clamped_basis(key):
    """(lam ascending, X [n_free modes, n] rows, zero on the clamp): ALL eigenpairs of (K, DENSITY M) clamped at clamp_vars(key), M-orthonormal at
    DENSITY (dense eigh; the small meshes only)."""
    K, M = U.pencil(key)
    free = H.free_of(key)
    lam, Xf = scipy.linalg.eigh(K[free][:, free].toarray(), H.DENSITY * M[free][:, free].toarray())
    X = np.zeros((len(lam), K.shape[0]))
    X[:, free] = Xf.T
    lam.setflags(write=False)
    X.setflags(write=False)
    return lam, X


@functools.lru_cache(maxsize=None)
def static_solution(key, kind="complex", clamped=True):
    """u_s of K u_s = f^ on the free variables for load(key, kind): the complex direct solve at zK = 1, zM = 0."""
    u = H.direct_solve(key, 1.0, 0.0, H.load(key, kind, clamped), clamped)
    u.setflags(write=False)
    return u


def denominators(lam, w, aR, bR, eta, zeta=None, dtype=np.float64):
    """d_j(w), complex, in the precision of dtype (np.float64 or np.longdouble)."""
    ct = np.clongdouble if dtype == np.longdouble else np.complex128
    lam = np.asarray(lam, dtype=dtype)
    w, aR, bR, eta = dtype(w), dtype(aR), dtype(bR), dtype(eta)
    d = (lam * (1 + 1j * ct(eta + w * bR))).astype(ct) - w * w + 1j * ct(w * aR)
    if zeta is not None:
        d = d + 2j * (np.asarray(zeta, dtype=dtype) * np.sqrt(lam) * w).astype(ct)
    return d


def modal_response(lam, X, f, omegas, aR=0.0, bR=0.0, eta=0.0, zeta=None, u_s=None, dtype=np.float64):
    """(u^ [nFreq, n], q [nFreq, m]) of the formula above for the modes (lam, rows of X); u_s: the static solution (None: no correction)."""
    ct = np.clongdouble if dtype == np.longdouble else np.complex128
    lam = np.asarray(lam, dtype=dtype)
    Xd = np.asarray(X, dtype=dtype)
    fd = np.asarray(f).astype(ct)
    g = Xd @ fd.real + 1j * (Xd @ fd.imag).astype(ct)
    r_s = None
    if u_s is not None:
        us = np.asarray(u_s).astype(ct)
        gl = g / lam
        r_s = us - (gl.real @ Xd + 1j * (gl.imag @ Xd).astype(ct))
    u = np.zeros((len(omegas), Xd.shape[1]), dtype=ct)
    q = np.zeros((len(omegas), len(lam)), dtype=ct)
    for k, w in enumerate(omegas):
        q[k] = g / denominators(lam, w, aR, bR, eta, zeta, dtype)
        u[k] = q[k].real @ Xd + 1j * (q[k].imag @ Xd).astype(ct)
        if r_s is not None:
            u[k] = u[k] + r_s / ct(1 + 1j * ct(dtype(eta) + dtype(w) * dtype(bR)))
    return u, q


def expand_bound(B, C):
    """Componentwise bound of the fma chain out[p][row] = sum_j B[j][row] C[j][p] over nb terms: (nb + 1) eps sum_j |B_j| |C_j|, [nPlanes, n]."""
    B, C = np.asarray(B, dtype=np.float64), np.asarray(C, dtype=np.float64)
    return (B.shape[0] + 1) * EPS * (np.abs(C).T @ np.abs(B))


def coords_bound(lam, X, f, omegas, aR=0.0, bR=0.0, eta=0.0, zeta=None, n_free=None):
    """[nFreq, m]: the bound on |q_j - g_j / d_j| of the device's modal coordinates: (n_free + 8) eps |1 / d_j| |phi_j|^T |f^| (the Gram sum over the
    rows, the complex division and the formation of d_j)."""
    X = np.asarray(X)
    n_free = X.shape[1] if n_free is None else n_free
    af = np.abs(X) @ (np.abs(np.real(f)) + np.abs(np.imag(f)))
    return np.array([(n_free + 8) * EPS * af / np.abs(denominators(lam, w, aR, bR, eta, zeta)) for w in omegas])


def response_bound(lam, X, f, omegas, aR=0.0, bR=0.0, eta=0.0, zeta=None, u_s=None, n_free=None, rtol_static=RTOL_STATIC):
    """[nFreq]: the bar on ||u^_dev - u^_ref||_2 (both planes) of a sweep against modal_response on the same (lam, X):
        eps [(n_free + 8) sum_j |1 / d_j| (|phi_j|^T |f^|) ||phi_j||_2  +  (nb + 1) || |B| |C| ||_2]   [+ 10 rtol ||u_s|| / |zK| with a correction],
    B = [Phi | r_re | r_im], C the real coefficient matrix of the frequency's two planes, nb = m + 2."""
    X = np.asarray(X)
    m = X.shape[0]
    cb = coords_bound(lam, X, f, omegas, aR, bR, eta, zeta, n_free)
    xn = np.linalg.norm(X, axis=1)
    u, q = modal_response(lam, X, f, omegas, aR, bR, eta, zeta, u_s)
    r_s = None
    if u_s is not None:
        g = X @ np.asarray(f)
        r_s = np.asarray(u_s) - (g / lam) @ X
    out = np.zeros(len(omegas))
    aX = np.abs(X)
    for k, w in enumerate(omegas):
        a_re = np.abs(q[k].real) @ aX
        a_im = np.abs(q[k].imag) @ aX
        if r_s is not None:
            iz = 1.0 / complex(1.0, eta + w * bR)
            a_re = a_re + np.abs(r_s.real) * abs(iz.real) + np.abs(r_s.imag) * abs(iz.imag)
            a_im = a_im + np.abs(r_s.real) * abs(iz.imag) + np.abs(r_s.imag) * abs(iz.real)
        out[k] = cb[k] @ xn + (m + 3) * EPS * np.sqrt(np.sum(a_re ** 2) + np.sum(a_im ** 2))
        if u_s is not None:
            out[k] += 10.0 * rtol_static * np.linalg.norm(u_s) / abs(complex(1.0, eta + w * bR))
    return out


def gram_bound(A, MB, n_free=None):
    """[na, nb]: (n + 1) eps sum_rows |A_i| |MB_j| for the Gram sums A (M B)^T (rows of A and of MB = the images of the rows of B)."""
    A, MB = np.abs(np.asarray(A)), np.abs(np.asarray(MB))
    n = A.shape[1] if n_free is None else n_free
    return (n + 1) * EPS * (A @ MB.T)
