"""Shared helpers of the frequency-response tests (tests/test_harmonic_reference.py, tests/test_gpu_harmonic.py, tests/test_cpp_harmonic.py): the
reference u^(w) of mfh_harmonic -- a complex sparse direct solve (splu) of

    Z(w) u^ = f^,   Z = zK K + zM M,   zK = 1 + i (eta + w bR),   zM = DENSITY (-w^2 + i w aR)

on the free variables of the oracle's pencil (K, M) of tests/modes_util.py -- its frequencies, damping cases and loads, and a numpy COCG with the two
preconditioners the device loop has (a stand-in whose deviation from the direct solve is what the device bars are set against). The library's reference
project has no harmonic solver, so the direct solve is the independent reference; every result is computed once per process (functools.lru_cache) and
handed out read-only."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import modes_util as U

DENSITY = 1.7
# (aR in units of omega_1, bR in units of 1 / omega_1, structural loss factor eta)
CASES = {"undamped": (0.0, 0.0, 0.0), "rayleigh": (0.1, 0.02, 0.0), "structural": (0.0, 0.0, 0.03)}
N_FREQ = 5


def _lu(A):
    return spla.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))


@functools.lru_cache(maxsize=None)
def natural_frequencies(key, clamped=True):
    """sqrt(lam / DENSITY), ascending: of the pencil clamped at clamp_vars(key), or the non-zero ones of the free body."""
    if clamped:
        lam = U.clamped_truth(key)[0]
    else:
        nz = 6 if U.fem_mesh(key).N == 3 else 3
        lam = U.free_truth(key)[0][nz:]
    w = np.sqrt(np.asarray(lam) / DENSITY)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def sweep_omegas(key):
    """{0, omega_1 / 2, mid(omega_2, omega_3), mid(omega_5, omega_6), mid(omega_8, omega_9)} of the clamped pencil: none on an eigenfrequency."""
    w = natural_frequencies(key)
    om = np.array([0.0, 0.5 * w[0], 0.5 * (w[1] + w[2]), 0.5 * (w[4] + w[5]), 0.5 * (w[7] + w[8])])
    om.setflags(write=False)
    return om


def damping(key, case, clamped=True):
    """((aR, bR), eta) in the units of the mesh."""
    a, b, eta = CASES[case]
    w1 = float(natural_frequencies(key, clamped)[0])
    return (a * w1, b / w1), eta


def coefficients(key, case, w, clamped=True):
    """(zK, zM) of Z = zK K + zM M with M at density 1."""
    (aR, bR), eta = damping(key, case, clamped)
    return complex(1.0, eta + w * bR), DENSITY * complex(-w * w, w * aR)


def free_of(key, clamped=True):
    n = U.pencil(key)[0].shape[0]
    return U.free_vars(key, U.clamp_vars(key)) if clamped else np.arange(n)


@functools.lru_cache(maxsize=None)
def load(key, kind="real", clamped=True):
    """A random load, zero on the clamp: "real", or "complex" (both planes random)."""
    n = U.pencil(key)[0].shape[0]
    rng = np.random.default_rng(17)
    keep = np.zeros(n)
    keep[free_of(key, clamped)] = 1.0
    f = rng.standard_normal(n) * keep
    if kind == "complex":
        f = f + 1j * rng.standard_normal(n) * keep
    f.setflags(write=False)
    return f


def direct_solve(key, zK, zM, f, clamped=True):
    """u^ (full length, zero on the clamp) of (zK K + zM M) u^ = f on the free variables by a complex splu."""
    K, M = U.pencil(key)
    free = free_of(key, clamped)
    Z = (zK * K[free][:, free] + zM * M[free][:, free]).astype(np.complex128)
    u = np.zeros(K.shape[0], dtype=np.complex128)
    u[free] = _lu(Z).solve(np.asarray(f, dtype=np.complex128)[free])
    return u


@functools.lru_cache(maxsize=None)
def reference(key, case, kind="real", omegas=None, clamped=True):
    """[nFreq, n] complex: the direct solves at sweep_omegas(key) (or the tuple omegas) for load(key, kind)."""
    om = sweep_omegas(key) if omegas is None else np.asarray(omegas)
    f = load(key, kind, clamped)
    out = np.array([direct_solve(key, *coefficients(key, case, float(w), clamped), f, clamped) for w in om])
    out.setflags(write=False)
    return out


def rel_l2(a, b):
    """||a - b||_2 / ||b||_2 over both planes."""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- the CPU stand-in of the device loop
def block_jacobi(A, d):
    """The inverse of the d x d diagonal blocks of the real symmetric A (rows grouped d at a time), as a sparse matrix."""
    A = sp.csr_matrix(A)
    nb = A.shape[0] // d
    assert nb * d == A.shape[0]
    blocks = np.zeros((nb, d, d))
    for a in range(d):
        for b in range(d):
            blocks[:, a, b] = np.asarray(A[np.arange(nb) * d + a, np.arange(nb) * d + b]).reshape(-1)
    return sp.block_diag(list(np.linalg.inv(blocks)), format="csr")


def cocg(Z, b, precond, rtol, maxit=20000):
    """Preconditioned COCG on the complex symmetric Z from x = 0: the PCG recurrence with x^T y. precond: r -> B r for a real SPD B (applied to
    the two planes by linearity). Stops at ||r||_2 <= rtol ||b||_2. Returns (x, iterations or -1, the recurrence's final ||r|| / ||b||, the
    smallest |p^T Z p| / (||p|| ||Z p||) seen)."""
    x = np.zeros_like(b, dtype=np.complex128)
    r = b.astype(np.complex128).copy()
    nb = np.linalg.norm(b)
    z = precond(r)
    p = z.copy()
    rho = r @ z
    worst = np.inf
    for it in range(maxit + 1):
        if np.linalg.norm(r) <= rtol * nb:
            return x, it, np.linalg.norm(r) / nb, worst
        if it == maxit:
            break
        q = Z @ p
        mu = p @ q
        worst = min(worst, abs(mu) / (np.linalg.norm(p) * np.linalg.norm(q)))
        alpha = rho / mu
        x += alpha * p
        r -= alpha * q
        z = precond(r)
        rho_new = r @ z
        p = z + (rho_new / rho) * p
        rho = rho_new
    return x, -1, np.linalg.norm(r) / nb, worst


@functools.lru_cache(maxsize=None)
def standin_runs(key, case, precond, rtol=1e-12):
    """One COCG per test frequency (cold start) with precond "Kinv" (exact K^-1, the stand-in of the V-cycle) or "jacobi" (block-Jacobi of
    K + w^2 DENSITY M). Returns a list of dicts: iterations, err (rel-L2 against the direct solve), true_res, min_pZp."""
    K, M = U.pencil(key)
    free = free_of(key)
    Kf, Mf = K[free][:, free].tocsr(), M[free][:, free].tocsr()
    d = U.fem_mesh(key).N
    f = load(key)[free].astype(np.complex128)
    ref = reference(key, case)
    kinv = _lu(Kf).solve if precond == "Kinv" else None
    out = []
    for k, w in enumerate(sweep_omegas(key)):
        zK, zM = coefficients(key, case, float(w))
        Z = (zK * Kf + zM * Mf).tocsr()
        if kinv is not None:
            B = lambda r: kinv(np.ascontiguousarray(r.real)) + 1j * kinv(np.ascontiguousarray(r.imag))
        else:
            D = block_jacobi(Kf + (w * w * DENSITY) * Mf, d)
            B = lambda r, D=D: D @ r
        x, its, _, worst = cocg(Z, f, B, rtol)
        out.append(dict(iterations=its, err=rel_l2(x, ref[k][free]), true_res=float(np.linalg.norm(f - Z @ x) / np.linalg.norm(f)), min_pZp=float(worst)))
    return out
