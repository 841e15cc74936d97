"""Shared helpers of the modal-transient tests (tests/test_modal_transient_reference.py, tests/test_gpu_modal_march.py,
tests/test_gpu_modal_transient.py, tests/test_cpp_modal_transient.py). None of it touches the library under test.

    q'' + c q' + lam q = g a(t),  a piecewise linear between a_n at n dt:
    [q ; q']_{n+1} = A [q ; q']_n + g (b0 a_n + b1 (a_{n+1} - a_n) / dt),
    [A | b0 b1] = the first two rows of exp(dt [[0,1,0,0],[-lam,-c,1,0],[0,0,0,1],[0,0,0,0]])

* mp_coeffs: the eight coefficients {A11, A12, b0_q, b1_q, A21, A22, b0_v, b1_v} from mpmath's matrix exponential at 50 digits, rounded to double;
* twin: the recurrence in numpy, float64 or np.longdouble, on any coefficient table; twin_defect: the distance of the two;
* dense_exact: the exact solution of the semi-discrete system M u'' + C u' + K u = f a(t) on a small clamped mesh: scipy's expm of the first-order
  system augmented by the two load states (a, s), one step matrix applied repeatedly.
Every reference is computed once per process (functools.lru_cache) and handed out read-only."""
import functools

import mpmath
import numpy as np
import scipy.linalg

import harmonic_util as H
import modal_util as MU
import modes_util as U

EPS = U.EPS
DENSITY = H.DENSITY
KEY56 = (2, 1)           # the 56-unknown clamped fixture of modal_util (asserted in fixture56)
# The worst distance of the float64 twin on the full basis from dense_exact, max_n ||u_n - u_n^exact||_2 / max_n ||u_n^exact||_2 over the nine cases of
# tests/test_modal_transient_reference.py::test_twin_is_the_dense_exact_solution, as that test printed it (it asserts that the figure still holds).
# The device run on the full basis is held to ten times this (tests/test_gpu_modal_transient.py).
TWIN_DENSE_WORST = 1.3e-13


@functools.lru_cache(maxsize=None)
def mp_coeffs(lam, c, dt):
    """The eight coefficients of one mode, mpmath at 50 digits rounded to double."""
    with mpmath.workdps(50):
        lam_, c_, dt_ = mpmath.mpf(float(lam)), mpmath.mpf(float(c)), mpmath.mpf(float(dt))
        N = mpmath.matrix([[0, 1, 0, 0], [-lam_, -c_, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]]) * dt_
        E = mpmath.expm(N, method="taylor")
        out = np.array([float(E[0, 0]), float(E[0, 1]), float(E[0, 2]), float(E[0, 3]), float(E[1, 0]), float(E[1, 1]), float(E[1, 2]), float(E[1, 3])])
    out.setflags(write=False)
    return out


def mp_table(lam, c, dt):
    """[m, 8]: mp_coeffs per mode."""
    return np.array([mp_coeffs(float(l), float(cc), float(dt)) for l, cc in zip(lam, c)])


def natural_scale(lam, c, dt):
    """S of the acceptance bar of the coefficients, in the order of the eight: [[1, h, h^2, h^2 dt], [1/h, 1, h, h^2]], h = min(dt, 1 / max(omega, c))."""
    w = max(np.sqrt(lam), c)
    h = min(dt, 1.0 / w) if w > 0 else dt
    return np.array([1.0, h, h * h, h * h * dt, 1.0 / h, 1.0, h, h * h])


def mode_damping(lam, aR=0.0, bR=0.0, zeta=None):
    """c_j = aR + bR lam_j + 2 zeta_j sqrt(lam_j), formed as the library forms it."""
    lam = np.asarray(lam, dtype=np.float64)
    c = aR + bR * lam
    if zeta is not None:
        c = c + 2.0 * np.broadcast_to(np.asarray(zeta, dtype=np.float64), lam.shape) * np.sqrt(lam)
    return c


def twin(coef, g, amp, dt, q0=None, v0=None, dtype=np.float64):
    """(Q, V) [n_steps + 1, m]: the recurrence on the coefficient table coef [m, 8] in the precision of dtype; row 0 is the start state."""
    coef = np.asarray(coef, dtype=dtype)
    g = np.asarray(g, dtype=dtype)
    amp = np.asarray(amp, dtype=dtype)
    dt = dtype(dt)
    m, rows = coef.shape[0], amp.size
    A11, A12, b0q, b1q, A21, A22, b0v, b1v = (coef[:, k] for k in range(8))
    Q, V = np.zeros((rows, m), dtype=dtype), np.zeros((rows, m), dtype=dtype)
    q = np.zeros(m, dtype=dtype) if q0 is None else np.asarray(q0, dtype=dtype).copy()
    v = np.zeros(m, dtype=dtype) if v0 is None else np.asarray(v0, dtype=dtype).copy()
    Q[0], V[0] = q, v
    pq, rq, pv, rv = g * b0q, g * b1q, g * b0v, g * b1v
    for r in range(1, rows):
        a0, s = amp[r - 1], (amp[r] - amp[r - 1]) / dt
        lq, lv = rq * s + pq * a0, rv * s + pv * a0
        q, v = A11 * q + (A12 * v + lq), A21 * q + (A22 * v + lv)
        Q[r], V[r] = q, v
    return Q, V


def rel_max(A, B):
    """max over the columns (modes) of max_n |A - B| / max_n |B| (a column of B that vanishes: its absolute figure): every mode counts on its own
    scale, however large another one grows."""
    A, B = np.asarray(A), np.asarray(B)
    if A.size == 0:
        return 0.0
    s = np.abs(B).max(axis=0)
    return float((np.abs(A - B).max(axis=0) / np.where(s > 0, s, 1.0)).max())


def twin_defect(coef, g, amp, dt, q0=None, v0=None):
    """(defect, Q, V of the long-double twin): the float64 twin against the long-double one on the same (float64) table, the larger of
    rel_max over the q rows and over the q' rows."""
    Q64, V64 = twin(coef, g, amp, dt, q0, v0)
    QL, VL = twin(coef, g, amp, dt, q0, v0, dtype=np.longdouble)
    return max(rel_max(Q64, QL), rel_max(V64, VL)), QL, VL


def energies_of(lam, g, amp, Q, V):
    """[rows, 3]: 1/2 sum q'^2, 1/2 sum lam q^2, a sum g q."""
    return np.stack([0.5 * np.sum(V * V, axis=1), 0.5 * np.sum(lam * Q * Q, axis=1), amp * (Q @ g)], axis=1)


# ---------------------------------------------------------------- the dense exact solution
@functools.lru_cache(maxsize=None)
def fixture56():
    """(Kf, rho Mf, free, lam, X) of the 56-unknown clamped fixture, dense."""
    K, M = U.pencil(KEY56)
    free = H.free_of(KEY56)
    assert len(free) == 56 or K.shape[0] == 56
    lam, X = MU.clamped_basis(KEY56)
    return K[free][:, free].toarray(), DENSITY * M[free][:, free].toarray(), free, lam, X


def dense_exact(f, amp, dt, aR=0.0, bR=0.0, zeta=None, u0=None, v0=None):
    """U [n_steps + 1, n]: the exact solution of rho M u'' + C u' + K u = f a(t) on fixture56, a piecewise linear, C = aR rho M + bR K or
    rho M Phi diag(2 zeta sqrt(lam)) Phi^T rho M."""
    Kf, Mf, free, lam, X = fixture56()
    nf = len(free)
    C = aR * Mf + bR * Kf
    if zeta is not None:
        MP = Mf @ X[:, free].T
        C = C + MP @ np.diag(2.0 * np.broadcast_to(zeta, lam.shape) * np.sqrt(lam)) @ MP.T
    G = np.zeros((2 * nf + 2, 2 * nf + 2))
    G[:nf, nf:2 * nf] = np.eye(nf)
    G[nf:2 * nf, :nf] = -np.linalg.solve(Mf, Kf)
    G[nf:2 * nf, nf:2 * nf] = -np.linalg.solve(Mf, C)
    G[nf:2 * nf, 2 * nf] = np.linalg.solve(Mf, np.asarray(f)[free])
    G[2 * nf, 2 * nf + 1] = 1.0
    E = scipy.linalg.expm(dt * G)[:2 * nf]
    amp = np.asarray(amp, dtype=np.float64)
    y = np.zeros(2 * nf + 2)
    if u0 is not None:
        y[:nf] = np.asarray(u0)[free]
    if v0 is not None:
        y[nf:2 * nf] = np.asarray(v0)[free]
    Us = np.zeros((amp.size, X.shape[1]))
    Us[0, free] = y[:nf]
    for r in range(1, amp.size):
        y[2 * nf], y[2 * nf + 1] = amp[r - 1], (amp[r] - amp[r - 1]) / dt
        y[:2 * nf] = E @ y
        Us[r, free] = y[:nf]
    return Us


DAMPING_CASES = ("undamped", "rayleigh", "zeta")


def damping_case(key, case, m=None):
    """(aR, bR, zeta) of a named case in the units of the mesh: Rayleigh 0.1 omega_1 / 0.02 / omega_1 as in harmonic_util, or zeta_j cycling through
    {0.01, 0.03, 0.08} over the modes."""
    if case == "undamped":
        return 0.0, 0.0, None
    if case == "rayleigh":
        (aR, bR), _ = H.damping(key, "rayleigh")
        return aR, bR, None
    lam = MU.clamped_basis(key)[0]
    m = len(lam) if m is None else m
    return 0.0, 0.0, np.array([0.01, 0.03, 0.08])[np.arange(m) % 3]


def loads(key, n_steps=200):
    """{name: (dt, amp)}: a step, a ramp over the run and a sine at omega_3, all at 12 points per SHORTEST period of the clamped pencil."""
    lam = MU.clamped_basis(key)[0]
    dt = 2.0 * np.pi / np.sqrt(lam[-1]) / 12.0
    t = dt * np.arange(n_steps + 1)
    return {"step": (dt, np.ones(n_steps + 1)), "ramp": (dt, t / t[-1]), "sine": (dt, np.sin(np.sqrt(lam[2]) * t))}


def modal_fields(X, Q, r_s=None, amp=None):
    """U [rows, n] = Q X (+ amp r_s) in float64."""
    Uo = np.asarray(Q, dtype=np.float64) @ np.asarray(X)
    if r_s is not None:
        Uo = Uo + np.outer(amp, r_s)
    return Uo
