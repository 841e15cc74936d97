"""Shared helpers of the many-modes tests (tests/test_modes_many_reference.py, tests/test_gpu_modes_many.py): the dense truth of the pencil restricted
to the M-orthogonal complement of a set Q, the fixtures' free blocks as dense matrices, and the bars of tests/test_gpu_modes.py. Everything is
computed once per process (functools.lru_cache) and handed out read-only; the meshes and the pencil come from tests/modes_util.py."""
import functools

import numpy as np
import scipy.linalg

import modes_util as U

EPS = U.EPS


def clamp_axis(key):
    return 2 if key == U.BAR else 0


@functools.lru_cache(maxsize=None)
def dense_clamped(key):
    """(Kff, Mff, free variables, cond2(Mff)) as dense arrays: the pencil of a small fixture clamped at clamp_vars(key, clamp_axis(key))."""
    K, M = U.pencil(key)
    f = U.free_vars(key, U.clamp_vars(key, clamp_axis(key)))
    Kf, Mf = K[f][:, f].toarray(), M[f][:, f].toarray()
    for a in (Kf, Mf, f):
        a.setflags(write=False)
    return Kf, Mf, f, float(np.linalg.cond(Mf))


@functools.lru_cache(maxsize=None)
def dense_spectrum(key, free=False):
    """(lam ascending, X columns, cond2(M), the orthonormality defect of scipy's vectors): every eigenpair of the clamped (or free-free) pencil."""
    if free:
        K, M = U.pencil(key)
        Kf, Mf = K.toarray(), M.toarray()
        cond = float(np.linalg.cond(Mf))
    else:
        Kf, Mf, _, cond = dense_clamped(key)
    lam, X = scipy.linalg.eigh(Kf, Mf)
    defect = float(np.abs(X.T @ (Mf @ X) - np.eye(X.shape[1])).max())
    lam.setflags(write=False); X.setflags(write=False)
    return lam, X, cond, defect


def restricted_truth(Kf, Mf, Q):
    """Eigenvalues (ascending) and vectors of K x = lam M x restricted to {x: Q^T M x = 0}: dense eigh on a null-space basis of (M Q)^T.
    Q: [n, nq], full rank."""
    N = scipy.linalg.null_space((Mf @ Q).T)
    assert N.shape[1] == Kf.shape[0] - Q.shape[1], "Q is rank deficient"
    lam, Y = scipy.linalg.eigh(N.T @ Kf @ N, N.T @ Mf @ N)
    return lam, N @ Y


def penalised_truth(Kf, Mf, Q, sigma):
    """The same spectrum from eigh(K + sigma M Q Q^T M, M): the directions of Q are moved up by about sigma (Q M-orthonormal: exactly, where Q
    spans an invariant subspace), the complement keeps its eigenvalues up to O(1 / sigma)."""
    MQ = Mf @ Q
    return scipy.linalg.eigh(Kf + sigma * (MQ @ MQ.T), Mf, eigvals_only=True)


def eig_bar(cond, rtol, lam):
    """|lambda~ - lambda| <= sqrt(cond2(M)) rtol lambda: the bar of tests/test_gpu_modes.py."""
    return np.sqrt(cond) * rtol * np.asarray(lam)


def random_set(n, nq, seed):
    Q = np.random.default_rng(seed).standard_normal((n, nq))
    Q.setflags(write=False)
    return Q


def m_orthonormalise(Q, Mf):
    return U.m_orthonormalise(Q, Mf)
