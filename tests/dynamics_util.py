"""Shared helpers of the transient-dynamics tests (tests/test_dynamics_reference.py, tests/test_gpu_dynamics.py, tests/test_cpp_dynamics.py): the
reference recurrence of mfh_newmark -- the Newmark scheme on the oracle's pencil (K, M) of tests/modes_util.py with sparse direct solves (splu) --
its inputs, and the closed forms it is checked against. The library's reference project has no time integrator, so this recurrence is the
independent reference; every run is computed once per process (functools.lru_cache) and handed out read-only.

    u~ = u + dt v + dt^2 (1/2 - beta) a          v~ = v + dt (1 - gamma) a
    A u+ = g+ f + M u~ / (beta dt^2) + C (gamma / (beta dt) u~ - v~),     A = K + gamma / (beta dt) C + M / (beta dt^2),  C = aR M + bR K
    a+ = (u+ - u~) / (beta dt^2)                 v+ = v~ + gamma dt a+
on the free variables, M = density x the consistent vector mass matrix; a0 from M a0 = g0 f - C v0 - K u0 unless given."""
import functools

import numpy as np
import scipy.sparse.linalg as spla

import modes_util as U

DENSITY = 1.7


def _lu(A):
    return spla.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))


def newmark_direct(K, M, free, dt, n_steps, u0, v0, f=None, amplitude=None, density=1.0, damping=(0.0, 0.0), beta=0.25, gamma=0.5, a0=None,
                   solve_A=None):
    """The recurrence on full-length vectors (zero on the fixed variables). Returns (U, V, A, E): the states of the steps 0 .. n_steps and the
    energies [n_steps + 1, 3] = 1/2 v.Mv, 1/2 u.Ku, g f.u. solve_A (optional): replaces the direct solve with A (b -> x)."""
    n = K.shape[0]
    Kf, Mf = K[free][:, free].tocsr(), (density * M[free][:, free]).tocsr()
    aR, bR = damping
    Cf = aR * Mf + bR * Kf
    g = np.ones(n_steps + 1) if amplitude is None else np.asarray(amplitude, dtype=np.float64)
    ff = np.zeros(len(free)) if f is None else np.asarray(f, dtype=np.float64)[free]
    u, v = np.asarray(u0, dtype=np.float64)[free].copy(), np.asarray(v0, dtype=np.float64)[free].copy()
    if a0 is None:
        rhs = g[0] * ff - Cf @ v - Kf @ u
        a = _lu(Mf).solve(rhs) if np.any(rhs) else np.zeros_like(rhs)
    else:
        a = np.asarray(a0, dtype=np.float64)[free].copy()
    if solve_A is None:
        solve_A = _lu(Kf + (gamma / (beta * dt)) * Cf + Mf / (beta * dt * dt)).solve
    Us, Vs, As = (np.zeros((n_steps + 1, n)) for _ in range(3))
    E = np.zeros((n_steps + 1, 3))

    def record(k):
        Us[k, free], Vs[k, free], As[k, free] = u, v, a
        E[k] = 0.5 * v @ (Mf @ v), 0.5 * u @ (Kf @ u), g[k] * (ff @ u)
    record(0)
    for k in range(1, n_steps + 1):
        ut = u + dt * v + dt * dt * (0.5 - beta) * a
        vt = v + dt * (1.0 - gamma) * a
        b = g[k] * ff + Mf @ (ut / (beta * dt * dt)) + Cf @ ((gamma / (beta * dt)) * ut - vt)
        u = solve_A(b)
        a = (u - ut) / (beta * dt * dt)
        v = vt + gamma * dt * a
        record(k)
    return Us, Vs, As, E


@functools.lru_cache(maxsize=None)
def omega1(key, clamped=True):
    """The lowest natural frequency of the pencil with density DENSITY: clamped at clamp_vars(key), or of the free body (first non-zero one)."""
    if clamped:
        lam = U.clamped_truth(key)[0][0]
    else:
        nz = 6 if U.fem_mesh(key).N == 3 else 3
        lam = U.free_truth(key)[0][nz]
    return float(np.sqrt(lam / DENSITY))


def free_of(key, clamped=True):
    n = U.pencil(key)[0].shape[0]
    return U.free_vars(key, U.clamp_vars(key)) if clamped else np.arange(n)


CASES = {"undamped": (0.0, 0.0), "damped": (0.1, 0.02)}     # Rayleigh coefficients in units of omega_1 and 1 / omega_1


@functools.lru_cache(maxsize=None)
def case_inputs(key, case, n_steps=100, clamped=True):
    """dict of the inputs of one reference run: dt = T_1 / 20, a random amplitude table, a random load, non-zero u0 and v0 (zero on the clamp).
    The mid mesh starts from u0 = 0 with g0 = 0 and no damping, so that a0 = 0 and no factorisation of M is needed."""
    K, _ = U.pencil(key)
    n = K.shape[0]
    w1 = omega1(key, clamped)
    rng = np.random.default_rng(11)
    free = free_of(key, clamped)
    keep = np.zeros(n)
    keep[free] = 1.0
    f = rng.standard_normal(n) * keep
    u0 = rng.standard_normal(n) * keep
    v0 = w1 * rng.standard_normal(n) * keep
    amp = rng.standard_normal(n_steps + 1)              # (drawn last: a shorter run is the start of the longer one)
    aR, bR = CASES[case]
    if key == U.MID:
        assert case == "undamped"
        u0 = np.zeros(n)
        amp[0] = 0.0
    d = dict(dt=2.0 * np.pi / w1 / 20.0, n_steps=n_steps, amplitude=amp, f=f, u0=u0, v0=v0, density=DENSITY, damping=(aR * w1, bR / w1), omega1=w1)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference_run(key, case, n_steps=100, clamped=True):
    """(U, V, A, E) of newmark_direct on case_inputs(key, case, n_steps, clamped)."""
    K, M = U.pencil(key)
    i = case_inputs(key, case, n_steps, clamped)
    out = newmark_direct(K, M, free_of(key, clamped), i["dt"], n_steps, i["u0"], i["v0"], i["f"], i["amplitude"], i["density"], i["damping"])
    for a in out:
        a.setflags(write=False)
    return out


def mode_shape(key, j):
    """(phi, omega): mode j of clamped_truth(key) as a full-length vector and its frequency under density DENSITY."""
    lam, X, _, _ = U.clamped_truth(key)
    n = U.pencil(key)[0].shape[0]
    phi = np.zeros(n)
    phi[free_of(key)] = X[:, j]
    return phi, float(np.sqrt(lam[j] / DENSITY))


def dispersion_closed_form(phi, omega, dt, n_steps):
    """u_n = phi cos(n theta), theta = 2 atan(omega dt / 2): the trapezoidal rule (beta = 1/4, gamma = 1/2) started from a mode shape at rest."""
    theta = 2.0 * np.arctan(0.5 * omega * dt)
    return np.cos(theta * np.arange(n_steps + 1))[:, None] * phi[None, :]


@functools.lru_cache(maxsize=None)
def dispersion_reference(key, j, n_steps=60):
    """(U of newmark_direct started from mode j, the closed form, the recurrence's own defect max_n ||U_n - closed_n|| / ||phi||)."""
    K, M = U.pencil(key)
    phi, om = mode_shape(key, j)
    dt = 2.0 * np.pi / omega1(key) / 20.0
    Us = newmark_direct(K, M, free_of(key), dt, n_steps, phi, np.zeros_like(phi), density=DENSITY)[0]
    closed = dispersion_closed_form(phi, om, dt, n_steps)
    return Us, closed, float(np.linalg.norm(Us - closed, axis=1).max() / np.linalg.norm(phi))


def rel_l2_rows(A, B):
    """max over the rows of ||A_k - B_k||_2 / ||B_k||_2 (rows of B that vanish: the absolute norm against the largest row)."""
    nb = np.linalg.norm(B, axis=1)
    nb = np.where(nb > 0, nb, nb.max() if nb.max() > 0 else 1.0)
    return float((np.linalg.norm(A - B, axis=1) / nb).max())
