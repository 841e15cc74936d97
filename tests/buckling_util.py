"""FP64 restatement of the geometric stiffness (mfh_set_prestress, mfh_geometric_apply, mfh_buckling; docs/design/04_16_buckling.md), in numpy and
independent of the library's tables:
    Kg = kron(sum_e int_e grad phi_i . sigma_e grad phi_j, I_dim)
with grad phi_i = sum_k (d phi_i / d l_k) grad l_k, the shape polynomials and the exact simplex integrals of volume_loads_util, grad l and the
volumes from volume_loads_util.geometry, sigma_e a flattened symmetric tensor with TENSOR shear entries (the layout of mfh_average_stress).
Also here: the column fixtures of the buckling tests, their dense truth eigh(Kg_ff, K_ff) with K from the CPU oracle, Euler's load factors, and
the componentwise rounding bound of the product y = Kg x. Every matrix is computed once per process (functools.lru_cache), handed out read-only."""
import functools
import math

import numpy as np
import scipy.linalg
import scipy.sparse as sp

import modes_util as U
import volume_loads_util as VL

from oracle import meshfem_oracle as O

EPS = U.EPS
COLUMNS = ["col3d-P1", "col3d-P2", "strip-P1", "strip-P2"]
# roundings one (element, i, j) contribution passes through on the device before it is added to its block: the barycentric gradients (a cross
# product or a 2 x 2 cofactor, one division: <= 6), the volume (<= 8), the pair coefficients times the volume (1), the two combinations of
# gradients (3 each), H (3 per entry), the contraction with sigma (dim^2 products and dim^2 - 1 adds: <= 17). 40 covers the chain with room to spare.
ROUNDINGS_PER_CONTRIBUTION = 40


# ------------------------------------------------------------------------------------------------ the restatement
def poly_derivative(p, k):
    out = []
    for c, e in p:
        if e[k]:
            d = list(e)
            d[k] -= 1
            out.append((c * e[k], tuple(d)))
    return out


@functools.lru_cache(maxsize=None)
def gradient_pair_coefficients(dim, deg):
    """Q[i, k, j, l] = int (d phi_i / d l_k)(d phi_j / d l_l) / vol"""
    P = VL.shape_polynomials(dim, deg)
    nv, npe = dim + 1, len(P)
    D = [[poly_derivative(p, k) for k in range(nv)] for p in P]
    Q = np.zeros((npe, nv, npe, nv))
    for i in range(npe):
        for k in range(nv):
            for j in range(npe):
                for l in range(nv):
                    if D[i][k] and D[j][l]:
                        Q[i, k, j, l] = VL.poly_integral(dim, VL.poly_mul(D[i][k], D[j][l]))
    Q.setflags(write=False)
    return Q


def unflatten(dim, s):
    F = np.array([[O.flatten_indices(dim, i, j) for j in range(dim)] for i in range(dim)])
    return np.asarray(s, dtype=np.float64)[..., F]


def flatten(dim, S):
    out = np.zeros(S.shape[:-2] + (dim * (dim + 1) // 2,))
    for i in range(dim):
        for j in range(i, dim):
            out[..., O.flatten_indices(dim, i, j)] = S[..., i, j]
    return out


def element_matrices(dim, deg, vol, gl, sigma):
    """[nE, npe, npe]: int_e grad phi_i . sigma_e grad phi_j"""
    S = np.einsum("eka,eab,elb->ekl", gl, unflatten(dim, sigma), gl)
    return vol[:, None, None] * np.einsum("ikjl,ekl->eij", gradient_pair_coefficients(dim, deg), S)


def _scalar_to_sparse(Ke, idx, n):
    npe = idx.shape[1]
    rows = np.repeat(idx, npe, axis=1).ravel()
    cols = np.tile(idx, (1, npe)).ravel()
    return sp.coo_matrix((Ke.ravel(), (rows, cols)), shape=(n, n)).tocsr()


def geometric_stiffness(dim, deg, elem_nodes, node_pos, sigma, dof=None, n_dof=None, scalar=False):
    """Kg as scipy CSR on interleaved displacement vectors (scalar=True: the one-value-per-node-pair matrix); dof / n_dof: a DoF map (P^T Kg P)"""
    en = np.asarray(elem_nodes, dtype=np.int64)
    vol, gl = VL.geometry(node_pos, en[:, :dim + 1])
    idx = en if dof is None else np.asarray(dof, dtype=np.int64)[en]
    n = len(node_pos) if n_dof is None else int(n_dof)
    Ks = _scalar_to_sparse(element_matrices(dim, deg, vol, gl, sigma), idx, n)
    return Ks if scalar else sp.csr_matrix(sp.kron(Ks, sp.identity(dim)))


def product_bound(dim, deg, elem_nodes, node_pos, sigma, x, dof=None, n_dof=None):
    """Componentwise worst-case rounding bound of y = Kg x computed in any order: (N_r + ROUNDINGS_PER_CONTRIBUTION) eps sum_j |Kg|_rj |x_j| per row
    r, where N_r counts the (element, i, j) summands that reach the row and |Kg| is the matrix with every summand taken by modulus -- sigma, the
    coefficients Q, and the geometry by its own componentwise perturbation bounds: |A^-1| |A| |A^-1| for the barycentric gradients (the inverse of
    the affine map A = [[1 .. 1], [p_0 .. p_d]]) and vol sum |A| o |A^-T| / (d + 1) for the volume."""
    en = np.asarray(elem_nodes, dtype=np.int64)
    P = np.asarray(node_pos, dtype=np.float64)[en[:, :dim + 1]]
    nE, nv, _ = P.shape
    A = np.concatenate([np.ones((nE, 1, nv)), np.swapaxes(P, 1, 2)], axis=1)
    Ai = np.linalg.inv(A)
    vol = np.abs(np.linalg.det(A)) / math.factorial(dim)
    gl_abs = np.matmul(np.matmul(np.abs(Ai), np.abs(A)), np.abs(Ai))[:, :, 1:]
    vol_abs = vol * np.einsum("eij,eji->e", np.abs(A), np.abs(Ai)) / nv
    S = np.einsum("eka,eab,elb->ekl", gl_abs, np.abs(unflatten(dim, sigma)), gl_abs)
    Ke = vol_abs[:, None, None] * np.einsum("ikjl,ekl->eij", np.abs(gradient_pair_coefficients(dim, deg)), S)
    idx = en if dof is None else np.asarray(dof, dtype=np.int64)[en]
    n = len(node_pos) if n_dof is None else int(n_dof)
    Kabs = _scalar_to_sparse(Ke, idx, n)
    count = np.asarray(_scalar_to_sparse(np.ones_like(Ke), idx, n).sum(axis=1)).ravel()
    xa = np.abs(np.asarray(x, dtype=np.float64)).reshape(n, -1)
    return ((count[:, None] + ROUNDINGS_PER_CONTRIBUTION) * EPS * (Kabs @ xa)).reshape(np.shape(x))


def random_symmetric_field(n_elem, dim, seed=3):
    """seeded symmetric tensors with entries in [-1, 1], flattened; indefinite on purpose"""
    s = np.random.default_rng(seed).uniform(-1.0, 1.0, (n_elem, dim * (dim + 1) // 2))
    s.setflags(write=False)
    return s


def uniform_field(n_elem, dim, S):
    s = np.tile(flatten(dim, np.asarray(S, dtype=np.float64)), (n_elem, 1))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def mesh_tables(key):
    """(elem_nodes, node_pos) of a modes_util mesh or a column fixture in the oracle's numbering (the library's own: the GPU tests assert it)"""
    m = fem_mesh(key)
    return np.asarray(m.elem_nodes, dtype=np.int64), np.asarray(m.node_pos, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def mesh_arrays(key):
    """(V, T, deg, V0) like modes_util.mesh_arrays, extended by the column fixtures: unit cells, every vertex moved by up to 0.05 per coordinate
    (seeded, uniform), the long axis last.
      col3d-P1  3 x 2 x 10 linear tets      col3d-P2  2 x 1 x 6 quadratic tets
      strip-P1  2 x 12 linear triangles     strip-P2  2 x 6 quadratic triangles (four triangles per cell)"""
    if key not in COLUMNS:
        return U.mesh_arrays(key)
    if key.startswith("col3d"):
        V0, T = O.grid_tet_mesh(3, 2, 10) if key.endswith("P1") else O.grid_tet_mesh(2, 1, 6)
    else:
        V0, Q = O.gen_grid_2d(2, 12) if key.endswith("P1") else O.gen_grid_2d(2, 6)
        V0, T = O.quad_tri_subdiv(V0, Q)
        V0 = np.ascontiguousarray(V0[:, :2])
    V0 = np.asarray(V0, dtype=np.float64)
    V = V0 + 0.05 * np.random.default_rng(12).uniform(-1.0, 1.0, V0.shape)
    deg = 1 if key.endswith("P1") else 2
    T = np.asarray(T)
    for a in (V, V0, T):
        a.setflags(write=False)
    return V, T, deg, V0


@functools.lru_cache(maxsize=None)
def fem_mesh(key):
    V, T, deg, _ = mesh_arrays(key)
    return O.FEMMesh(T, V, deg)


def long_axis(key):
    return mesh_arrays(key)[0].shape[1] - 1


@functools.lru_cache(maxsize=None)
def clamp_vars(key):
    """all variables of the nodes on the face (long axis = min) of the unperturbed grid; modes_util's face x = min on its own meshes"""
    if key not in COLUMNS:
        return U.clamp_vars(key)
    V, T, deg, V0 = mesh_arrays(key)
    ax = long_axis(key)
    pos0 = O.FEMMesh(T, V0, deg).node_pos
    nodes = np.nonzero(pos0[:, ax] == pos0[:, ax].min())[0]
    d = V.shape[1]
    v = (d * nodes[:, None] + np.arange(d)[None, :]).reshape(-1).astype(np.int64)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def stiffness(key):
    """the oracle's K (isotropic E = 1, nu = 0.3), scipy CSR, both triangles"""
    if key not in COLUMNS:
        return U.pencil(key)[0]
    V, T, deg, _ = mesh_arrays(key)
    m = fem_mesh(key)
    sim = O.Simulator(T, V, deg, mesh=m)
    sim.set_material_constant(O.ElasticityTensor.isotropic(m.N, U.E_MOD, U.NU))
    return sp.csr_matrix(sim.assembleStiffnessMatrix().sum_repeated().to_scipy_full_from_upper())


def axial_compression(key, magnitude=1.0):
    """sigma = -magnitude e_L (x) e_L per element, L the long axis"""
    en, pos = mesh_tables(key)
    d = pos.shape[1]
    S = np.zeros((d, d))
    S[d - 1, d - 1] = -magnitude
    return uniform_field(len(en), d, S)


def Kg_of(key, sigma):
    en, pos = mesh_tables(key)
    _, _, deg, _ = mesh_arrays(key)
    return geometric_stiffness(pos.shape[1], deg, en, pos, sigma)


def free_vars(key):
    n = stiffness(key).shape[0]
    keep = np.ones(n, dtype=bool)
    keep[clamp_vars(key)] = False
    return np.nonzero(keep)[0]


def dense_truth(key, sigma):
    """(mu ascending, X columns on the free variables, cond2(K_ff), eigh's own K-orthonormality defect) of Kg x = mu K x clamped at clamp_vars"""
    f = free_vars(key)
    Kf = stiffness(key)[f][:, f].toarray()
    Gf = Kg_of(key, sigma)[f][:, f].toarray()
    mu, X = scipy.linalg.eigh(Gf, Kf)
    defect = np.abs(X.T @ (Kf @ X) - np.eye(X.shape[1])).max()
    return mu, X, float(np.linalg.cond(Kf)), float(defect)


@functools.lru_cache(maxsize=None)
def column_truth(key):
    """dense_truth under unit axial compression"""
    return dense_truth(key, axial_compression(key))


def factors_of(mu):
    """load factors -1 / mu, +inf where mu is not negative beyond rounding"""
    mu = np.asarray(mu, dtype=np.float64)
    out = np.full(mu.shape, np.inf)
    neg = mu < -1e-12 * np.abs(mu).max()
    out[neg] = -1.0 / mu[neg]
    return out


def euler_factor(key):
    """Euler's first load factor of the clamped-free column of the UNPERTURBED grid under unit axial stress: pi^2 E I / (4 L^2) over the
    cross-section area, I about the weak axis; the 2D strip is a plane-stress beam of unit thickness"""
    V0 = mesh_arrays(key)[3]
    ext = V0.max(axis=0) - V0.min(axis=0)
    Lc, cross = ext[-1], np.sort(ext[:-1])
    h = cross[0]                                         # the thin direction
    area = float(np.prod(cross))
    I = area * h * h / 12.0
    return float(np.pi ** 2 * U.E_MOD * I / (4.0 * Lc ** 2) / area)


def host_residuals(K, Kg, mu, X):
    """||Kg x - mu K x||_2 / (|mu| ||K x||_2) per row of X"""
    KX, GX = K @ X.T, Kg @ X.T
    return np.linalg.norm(GX - KX * mu[None, :], axis=0) / (np.abs(mu) * np.linalg.norm(KX, axis=0))
