"""Vibrational modes without a device: the host Rayleigh-Ritz routine of mfh_modes (mfh_debug_sym_gen_eig: Cholesky reduction + cyclic Jacobi)
against scipy.linalg.eigh, a self-check of the references the GPU tests compare with (tests/modes_util.py), and the refusals of mfh_modes
that must happen before any device is touched."""
import numpy as np
import pytest
import scipy.linalg

import meshfem_amd as M
from meshfem_amd import _lib, grid

import modes_util as U

EPS = U.EPS


def _spd(rng, n, cond=None):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.logspace(0, -np.log10(cond), n) if cond else rng.uniform(0.5, 2.0, n)
    B = (Q * d) @ Q.T
    return 0.5 * (B + B.T)


def _pencils():
    rng = np.random.default_rng(7)
    out = []
    for n in (1, 2, 3, 17, 48, 72):
        A = rng.standard_normal((n, n))
        out.append(("random n=%d" % n, 0.5 * (A + A.T) + n * np.eye(n), _spd(rng, n)))
    # a triple eigenvalue: A = L diag(w) L^T with B = L L^T has exactly the eigenvalues w
    n = 17
    L = np.tril(rng.standard_normal((n, n))) + 4 * np.eye(n)
    w = np.sort(rng.uniform(1.0, 9.0, n))
    w[5] = w[6] = w[7]
    out.append(("triple eigenvalue", (L * w) @ L.T, L @ L.T))
    # cond(B) = 1e8, built the same way from a factor L = Q D^1/2 R of B = Q D Q^T (Q, R orthogonal, D from 1 down to 1e-8), so that the eigenvalues
    # are w. Why not an arbitrary A: the Cholesky factor of B carries a backward error of n eps ||B||, which moves an eigenvalue lambda with
    # B-normalised vector x by lambda x^T dB x <= lambda n eps cond(B) -- for |lambda| near ||A|| ||B^-1|| that is cond(B) times the bar below,
    # for scipy as for any method that factors B (measured on A = random + n I: scipy 2.2, this routine 3.7 away from a 60-digit
    # reference, bar 6e-5). With lambda = O(||A|| / ||B||) the two coincide and the bar is the attainable one.
    n = 48
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    R, _ = np.linalg.qr(rng.standard_normal((n, n)))
    L = (Q * np.sqrt(np.logspace(0, -8, n))) @ R
    w = np.sort(rng.uniform(1.0, 9.0, n))
    out.append(("cond(B) = 1e8", (L * w) @ L.T, L @ L.T))
    return out


PENCILS = _pencils()


@pytest.mark.parametrize("name,A,B", PENCILS, ids=[p[0] for p in PENCILS])
def test_sym_gen_eig_against_scipy(name, A, B):
    """Eigenvalues within n eps ||B^-1|| ||A|| (the backward-error bound of the reduction to standard form) of scipy.linalg.eigh(A, B);
    ||V^T B V - I||_max within 10 x the defect of scipy's own vectors on the pencil (Jacobi and LAPACK differ in the constant, not the order)."""
    A = 0.5 * (A + A.T)
    B = 0.5 * (B + B.T)
    n = len(A)
    c = M.Context(-1)
    w, V = c.debug_sym_gen_eig(A, B)
    c.close()
    w_ref, V_ref = scipy.linalg.eigh(A, B)
    bar = n * EPS * np.linalg.norm(np.linalg.inv(B), 2) * np.linalg.norm(A, 2)
    err = np.abs(w - w_ref).max()
    defect, defect_ref = np.abs(V.T @ B @ V - np.eye(n)).max(), np.abs(V_ref.T @ B @ V_ref - np.eye(n)).max()
    print("%s: eigenvalue error %.3e (bar %.3e), defect %.3e (scipy %.3e)" % (name, err, bar, defect, defect_ref))
    assert np.all(np.diff(w) >= 0)
    assert err <= bar
    assert defect <= 10 * defect_ref


def test_sym_gen_eig_refuses_an_indefinite_B():
    lib = _lib.load()
    A, B = np.eye(3), np.diag([1.0, -1.0, 1.0])
    w, V = np.empty(3), np.empty((3, 3))
    assert lib.mfh_debug_sym_gen_eig(3, _lib.ptr(A), _lib.ptr(B), _lib.ptr(w), _lib.ptr(V)) == _lib.ERR_INVALID
    assert lib.mfh_debug_sym_gen_eig(73, None, None, None, None) == _lib.ERR_INVALID


@pytest.mark.parametrize("key", U.SMALL, ids=lambda k: "%dD-P%d" % k)
def test_reference_pencils_small(key):
    """The dense truth of the small meshes: exactly 6 / 3 eigenvalues of the free-free pencil below 1e-9 lambda_7 (lambda_4), the rigid-body
    modes span that eigenspace, and doubling the density halves every eigenvalue."""
    K, Mm = U.pencil(key)
    m = U.fem_mesh(key)
    nz = 6 if m.N == 3 else 3
    lam, X, cond, _ = U.free_truth(key)
    assert np.sum(np.abs(lam) < 1e-9 * lam[nz]) == nz and lam[nz] > 0
    Z = U.m_orthonormalise(U.rigid_modes(m.node_pos), Mm)
    assert np.abs(K @ Z).max() <= 1e-12 * np.abs(K).max() * np.abs(Z).max()
    # Z lies in the span of the nz null vectors: its M-projection on them reproduces it
    X0 = X[:, :nz]
    assert np.abs(X0 @ (X0.T @ (Mm @ Z)) - Z).max() <= 1e-8 * np.abs(Z).max()
    lam2 = scipy.linalg.eigh(K.toarray(), 2.0 * Mm.toarray(), eigvals_only=True)
    assert np.abs(2.0 * lam2[nz:] - lam[nz:]).max() <= 1e-10 * lam[-1]
    # the clamp removes every rigid motion: K_ff is positive definite
    lamc, Xc, condc, defect = U.clamped_truth(key)
    assert lamc[0] > 1e-6 * lamc[-1] and condc >= 1 and defect < 1e-10


def test_reference_pencil_mid():
    """The shift-invert truth of the mid mesh (8 x 7 x 6 quadratic tets: 12 635 nodes with those on the diagonals of the hexahedra, 37 905 unknowns): the free-free pencil has 6 zeros below 1e-9 lambda_7,
    spanned by the rigid-body modes; the values are eigenvalues (residual check against the matrices themselves)."""
    key = U.MID
    K, Mm = U.pencil(key)
    assert K.shape[0] == 37905
    m = U.fem_mesh(key)
    lam, X, cond, _ = U.free_truth(key)
    assert np.sum(np.abs(lam) < 1e-9 * lam[6]) == 6
    Z = U.m_orthonormalise(U.rigid_modes(m.node_pos), Mm)
    X0 = X[:, :6]
    assert np.abs(X0 @ (X0.T @ (Mm @ Z)) - Z).max() <= 1e-7 * np.abs(Z).max()
    assert U.host_residuals(K, Mm, lam[6:], X[:, 6:].T).max() < 1e-9
    lamc, Xc, condc, _ = U.clamped_truth(key)
    assert U.host_residuals(K[:, U.free_vars(key, U.clamp_vars(key))][U.free_vars(key, U.clamp_vars(key))],
                            Mm[:, U.free_vars(key, U.clamp_vars(key))][U.free_vars(key, U.clamp_vars(key))], lamc, Xc.T).max() < 1e-9
    assert 1 < condc < 1e6 and 1 < cond < 1e6


def _host_ctx():
    V, T = grid.grid_tet_mesh(1, 1, 1)
    c = M.Context(-1)
    c.mesh_build(T, V, 1)
    return c


def test_modes_on_a_host_only_context_is_refused_like_numeric_work():
    """mfh_create(-1): the status tests/test_abi.py::test_host_only_context_refuses_numeric_work expects of every numeric entry point."""
    c = _host_ctx()
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes(2)
    assert ei.value.code == _lib.ERR_HIP
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes(2, free=True)
    assert ei.value.code == _lib.ERR_HIP
    c.close()


def test_modes_argument_refusals_touch_no_device():
    """nev 0 or 21, density <= 0 and null outputs: MFH_ERR_INVALID, decided before the device is asked for (a host-only context gets this
    status, not the MFH_ERR_HIP of the test above)."""
    import ctypes as C
    c = _host_ctx()
    n = 3 * c.n_dof
    for kw in (dict(nev=0), dict(nev=21), dict(nev=2, density=0.0), dict(nev=2, density=-1.0)):
        with pytest.raises(M.MeshFEMHipError) as ei:
            c.modes(**kw)
        assert ei.value.code == _lib.ERR_INVALID, kw
    lam, X = np.zeros(2), np.zeros((2, n))
    info = _lib.ModesInfo()
    lib = _lib.load()
    assert lib.mfh_modes(c.h, 2, 1.0, 0, 1e-6, 10, None, _lib.ptr(X), None, C.byref(info)) == _lib.ERR_INVALID
    assert lib.mfh_modes(c.h, 2, 1.0, 0, 1e-6, 10, _lib.ptr(lam), None, None, C.byref(info)) == _lib.ERR_INVALID
    assert lib.mfh_modes(c.h, 2, 1.0, 0, 1e-6, 10, _lib.ptr(lam), _lib.ptr(X), None, None) == _lib.ERR_HIP      # (info and residuals may be null)
    c.close()
