"""Shared helpers of the vibrational-mode tests (tests/test_modes_reference.py, tests/test_gpu_modes.py, tests/test_cpp_modes.py): the meshes,
the pencil (K, M) from the CPU oracle, the clamp, the rigid-body modes and the scipy truth. Every reference is computed once per process
(functools.lru_cache) and handed out read-only."""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import meshfem_oracle as O

E_MOD, NU = 1.0, 0.3
SMALL = [(2, 1), (2, 2), (3, 1), (3, 2)]
MID = "mid"
BAR = "bar"
EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def mesh_arrays(key):
    """(V, T, deg, V0): V0 = the unperturbed grid (the clamp is chosen on it). key: (dim, deg) = the _mesh(dim, deg) construction of
    tests/test_gpu_differential_operators.py; MID = 8 x 7 x 6 quadratic tets (37 905 unknowns); BAR = the unperturbed 2 x 2 x 6 linear bar."""
    if key == MID:
        V0, T = O.grid_tet_mesh(8, 7, 6)
        V = V0 + 0.04 * np.random.default_rng(1).standard_normal(V0.shape)        # (0.08 inverts an element among the 2 016)
        deg = 2
    elif key == BAR:
        V0, T = O.grid_tet_mesh(2, 2, 6)
        V, deg = V0.copy(), 1
    else:
        dim, deg = key
        if dim == 3:
            V0, T = O.grid_tet_mesh(3, 2, 2)
        else:
            V0, Q = O.gen_grid_2d(4, 3)
            V0, T = O.quad_tri_subdiv(V0, Q)
            V0 = V0[:, :2]
        V = V0 + 0.08 * np.random.default_rng(0).standard_normal(V0.shape)
    for a in (V, V0, T):
        a.setflags(write=False)
    return V, T, deg, V0


@functools.lru_cache(maxsize=None)
def fem_mesh(key):
    V, T, deg, _ = mesh_arrays(key)
    return O.FEMMesh(T, V, deg)


@functools.lru_cache(maxsize=None)
def pencil(key):
    """(K, M) as scipy CSR, both triangles, density 1: the oracle's stiffness matrix (isotropic E = 1, nu = 0.3) and the Kronecker expansion of its
    scalar mass triplets (MassMatrix::construct_vector_valued)."""
    V, T, deg, _ = mesh_arrays(key)
    m = fem_mesh(key)
    sim = O.Simulator(T, V, deg, mesh=m)
    sim.set_material_constant(O.ElasticityTensor.isotropic(m.N, E_MOD, NU))
    K = sp.csr_matrix(sim.assembleStiffnessMatrix().sum_repeated().to_scipy_full_from_upper())
    Ms = O.mass_triplets(m).sum_repeated().to_scipy_full_from_upper()
    M = sp.csr_matrix(sp.kron(Ms, sp.identity(m.N)))
    return K, M


@functools.lru_cache(maxsize=None)
def clamp_vars(key, axis=0):
    """Variables of all nodes on the face (coordinate `axis` = min) of the unperturbed grid."""
    V, T, deg, V0 = mesh_arrays(key)
    pos0 = O.FEMMesh(T, V0, deg).node_pos
    nodes = np.nonzero(pos0[:, axis] == pos0[:, axis].min())[0]
    d = V.shape[1]
    v = (d * nodes[:, None] + np.arange(d)[None, :]).reshape(-1).astype(np.int64)
    v.setflags(write=False)
    return v


def free_vars(key, fixed):
    n = pencil(key)[0].shape[0]
    keep = np.ones(n, dtype=bool)
    keep[np.asarray(fixed, dtype=np.int64)] = False
    return np.nonzero(keep)[0]


def rigid_modes(pos):
    """[n dim, 6 | 3]: translations and infinitesimal rotations about the centroid of the nodes."""
    n, d = pos.shape
    x = pos - pos.mean(axis=0)
    Z = np.zeros((n, d, 6 if d == 3 else 3))
    for a in range(d):
        Z[:, a, a] = 1.0
    if d == 3:
        Z[:, 1, 3], Z[:, 2, 3] = -x[:, 2], x[:, 1]
        Z[:, 0, 4], Z[:, 2, 4] = x[:, 2], -x[:, 0]
        Z[:, 0, 5], Z[:, 1, 5] = -x[:, 1], x[:, 0]
    else:
        Z[:, 0, 2], Z[:, 1, 2] = -x[:, 1], x[:, 0]
    return Z.reshape(n * d, -1)


def shift_invert_eigsh(A, M, sigma, k):
    """eigsh(A, k, M, sigma) in shift-invert mode with the factorisation of A - sigma M made here: SuperLU under a symmetric minimum-degree ordering
    (a sixth of the fill its default column ordering produces on these matrices: 4 s instead of 80 on the mid mesh)."""
    S = (A - sigma * M).tocsc() if sigma != 0.0 else A.tocsc()
    lu = spla.splu(S, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    op = spla.LinearOperator(S.shape, matvec=lu.solve, dtype=np.float64)
    lam, X = spla.eigsh(A.tocsc(), k=k, M=M.tocsc(), sigma=sigma, OPinv=op, which="LM", tol=1e-13)
    order = np.argsort(lam)
    return lam[order], X[:, order]


def cond_of_mass(M):
    """cond2 of a (well-conditioned) sparse mass matrix from its two extreme eigenvalues (Lanczos, no factorisation)."""
    hi = spla.eigsh(M, k=1, which="LA", return_eigenvectors=False, tol=1e-8)[0]
    lo = spla.eigsh(M, k=1, which="SA", return_eigenvectors=False, tol=1e-8)[0]
    return hi / lo


def m_orthonormalise(Z, M):
    L = np.linalg.cholesky(Z.T @ (M @ Z))
    return np.linalg.solve(L, Z.T).T


@functools.lru_cache(maxsize=None)
def clamped_truth(key, nev_max=9):
    """(lam ascending, X columns, cond2(M_ff), scipy's own orthonormality defect) of the pencil clamped at clamp_vars(key): dense eigh on the small
    meshes, shift-invert eigsh about 0 on the mid mesh (K_ff is positive definite)."""
    K, M = pencil(key)
    f = free_vars(key, clamp_vars(key))
    Kf, Mf = K[f][:, f], M[f][:, f]
    if key == MID:
        lam, X = shift_invert_eigsh(Kf, Mf, 0.0, nev_max)
        cond = cond_of_mass(Mf)
    else:
        lam, X = scipy.linalg.eigh(Kf.toarray(), Mf.toarray())
        cond = np.linalg.cond(Mf.toarray())
    defect = np.abs(X.T @ (Mf @ X) - np.eye(X.shape[1])).max()
    return lam, X, float(cond), float(defect)


@functools.lru_cache(maxsize=None)
def free_truth(key, nev_max=6):
    """(all computed lam ascending INCLUDING the 6 / 3 zeros, X, cond2(M), scipy's orthonormality defect) of the free-free pencil: dense on the
    small meshes; on the mid mesh eigsh with a small negative shift, so that K - sigma M is positive definite."""
    K, M = pencil(key)
    nz = 6 if fem_mesh(key).N == 3 else 3
    if key == MID:
        lam, X = shift_invert_eigsh(K, M, -1e-3, nz + nev_max)
        cond = cond_of_mass(M)
    else:
        lam, X = scipy.linalg.eigh(K.toarray(), M.toarray())
        cond = np.linalg.cond(M.toarray())
    defect = np.abs(X.T @ (M @ X) - np.eye(X.shape[1])).max()
    return lam, X, float(cond), float(defect)


def host_residuals(K, M, lam, X):
    """||K x - lam M x||_2 / (lam ||M x||_2) per row of X."""
    KX, MX = (K @ X.T), (M @ X.T)
    return np.linalg.norm(KX - MX * lam[None, :], axis=0) / (lam * np.linalg.norm(MX, axis=0))


def sign_rule_holds(X):
    at = np.abs(X).argmax(axis=1)
    return bool(np.all(X[np.arange(len(X)), at] > 0))
