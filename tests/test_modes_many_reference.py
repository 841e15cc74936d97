"""CPU side of mfh_modes_many: the numpy truth the GPU tests compare against is checked against two independent formulations, and every
MFH_ERR_INVALID refusal of the entry point is checked on a host-only context (they all come before any device work)."""
import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import _lib, grid

import modes_util as U
import modes_many_util as MU


@pytest.mark.parametrize("key", [(3, 1), (2, 2)], ids=lambda k: "%dD-P%d" % k)
def test_restricted_truth_against_the_penalised_pencil(key):
    """eigh on a null-space basis of (M Q)^T against eigh(K + sigma M Q Q^T M, M) with Q M-orthonormal and sigma = 1e8 lambda_max: the penalised
    pencil keeps the complement's eigenvalues up to a relative O(lambda / sigma) and puts nq eigenvalues near sigma."""
    Kf, Mf, _, _ = MU.dense_clamped(key)
    n, nq = Kf.shape[0], 7
    Q = MU.m_orthonormalise(MU.random_set(n, nq, 3), Mf)
    lam, X = MU.restricted_truth(Kf, Mf, Q)
    assert len(lam) == n - nq
    assert np.abs(Q.T @ Mf @ X).max() <= 1e-10
    top = MU.dense_spectrum(key)[0][-1]
    sigma = 1e8 * top
    pen = MU.penalised_truth(Kf, Mf, Q, sigma)
    assert np.all(pen[n - nq:] >= 0.5 * sigma)
    # second-order perturbation: the coupling K_cq^2 / sigma, relative to lambda at most lambda_max^2 / (sigma lambda_min)
    tol = 10 * top * top / (sigma * lam[0]) + 1e-9
    assert np.abs(pen[:n - nq] - lam).max() <= tol * lam.max()
    assert np.abs(pen[:20] - lam[:20]).max() <= 1e-6 * lam[20]


@pytest.mark.parametrize("key", [(3, 1), (2, 2), U.BAR], ids=str)
def test_restricted_truth_with_exact_eigenvectors(key):
    """Q = the first nq eigenvectors: the restricted spectrum is the plain one shifted by nq."""
    Kf, Mf, _, _ = MU.dense_clamped(key)
    ref, X, _, _ = MU.dense_spectrum(key)
    for nq in (1, 8):
        lam, _ = MU.restricted_truth(Kf, Mf, X[:, :nq])
        assert np.abs(lam - ref[nq:]).max() <= 1e-9 * ref[-1]
        assert np.abs(lam[:30] - ref[nq:nq + 30]).max() <= 1e-9 * ref[nq + 30]


@pytest.fixture(scope="module")
def host_ctx():
    V, T = grid.grid_tet_mesh(2, 1, 1)
    c = M.Context(-1)
    c.mesh_build(T, V, 1)
    yield c
    c.close()


def _refused(c, **kw):
    args = dict(nev=2, density=1.0, free=True, locked=None, lambda_max=None, batch=0, rtol=1e-6, lock_factor=0.1, maxit=10)
    args.update(kw)
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes_many(args.pop("nev"), **args)
    return ei.value.code


def test_invalid_refusals_need_no_device(host_ctx):
    c = host_ctx
    n = c.bs * c.n_dof                 # 36 variables, 6 rigid modes
    Q = np.random.default_rng(0).standard_normal((3, n))
    bad = Q.copy()
    bad[1, 5] = np.inf
    nan = Q.copy()
    nan[2, 0] = np.nan
    cases = [dict(nev=0), dict(nev=-1), dict(nev=257), dict(nev=254, locked=Q), dict(batch=21), dict(batch=-1), dict(maxit=0),
             dict(nev=n - 6 + 1), dict(nev=n - 6 - 3 + 1, locked=Q), dict(nev=n + 1, free=False),
             dict(locked=bad), dict(locked=nan),
             dict(lock_factor=1.5), dict(lock_factor=-0.1), dict(lock_factor=float("nan")),
             dict(rtol=0.0), dict(rtol=-1e-6), dict(rtol=float("nan")), dict(density=0.0), dict(lambda_max=float("nan"))]
    for kw in cases:
        assert _refused(c, **kw) == _lib.ERR_INVALID, kw
    # 256 locked rows are out of range whatever nev is
    assert _refused(c, nev=1, locked=np.zeros((256, n))) == _lib.ERR_INVALID
    # a valid call gets as far as the device check: the refusals above came before it
    assert _refused(c) == _lib.ERR_HIP
    assert _refused(c, nev=n - 6 - 3, locked=Q) == _lib.ERR_HIP
    assert _refused(c, lock_factor=1.0, lambda_max=float("inf")) == _lib.ERR_HIP


def test_raw_call_refuses_null_arguments(host_ctx):
    import ctypes as C
    c = host_ctx
    n = c.bs * c.n_dof
    lam, X = np.zeros(2), np.zeros((2, n))
    prm = _lib.ModesManyParams(2, 0, 0, 0, 10, 0, 1.0, 1e-6, 0.0, 0.0)
    info = _lib.ModesManyInfo()
    f = c.lib.mfh_modes_many
    assert f(c.h, None, None, _lib.ptr(lam), _lib.ptr(X), None, C.byref(info)) == _lib.ERR_INVALID
    assert f(c.h, C.byref(prm), None, None, _lib.ptr(X), None, C.byref(info)) == _lib.ERR_INVALID
    assert f(c.h, C.byref(prm), None, _lib.ptr(lam), None, None, C.byref(info)) == _lib.ERR_INVALID
    prm.nLocked = 2                    # rows of Q announced, none given
    assert f(c.h, C.byref(prm), None, _lib.ptr(lam), _lib.ptr(X), None, C.byref(info)) == _lib.ERR_INVALID
    prm.nLocked, prm.reserved = 0, 1
    assert f(c.h, C.byref(prm), None, _lib.ptr(lam), _lib.ptr(X), None, C.byref(info)) == _lib.ERR_INVALID
    prm.reserved, prm.flags = 0, 2
    assert f(c.h, C.byref(prm), None, _lib.ptr(lam), _lib.ptr(X), None, C.byref(info)) == _lib.ERR_INVALID
    prm.flags = 0
    assert f(c.h, C.byref(prm), None, _lib.ptr(lam), _lib.ptr(X), None, None) == _lib.ERR_HIP          # info may be null
