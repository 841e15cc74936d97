"""FP64 restatement of the per-element density (mfh_set_density, mfh_mass_apply, mfh_mass_properties; docs/design/04_15_density.md), in numpy
and independent of the library's tables:
    M_rho = kron(sum_e rho_e vol_e m_ij, I_dim)       m_ij = int phi_i phi_j / vol from the exact simplex integrals of volume_loads_util,
                                                      vol from volume_loads_util.geometry
and the mass properties of the straight-sided body from the closed forms per element with vertices p_k:
    int 1 = vol,   int x = vol mean(p_k),   int (x - c)(x - c)^T = vol / ((d+1)(d+2)) (sum_k q_k q_k^T + (sum_k q_k)(sum_k q_k)^T),  q_k = p_k - c.
Every matrix is computed once per process (functools.lru_cache) and handed out read-only."""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp

import modes_util as U
import volume_loads_util as VL

FIELDS = ["bimaterial", "random"]


@functools.lru_cache(maxsize=None)
def mesh_tables(key):
    """(elem_nodes [nE, npe], node_pos [nNode, dim]) of the oracle's FEM mesh (the library's own numbering: the GPU tests assert it)"""
    m = U.fem_mesh(key)
    en = np.asarray(m.elem_nodes, dtype=np.int64)
    pos = np.asarray(m.node_pos, dtype=np.float64)
    return en, pos


def density_field(name, elem_nodes, node_pos, dim):
    """bimaterial: 1 where the element centroid has x < mid (the middle of the body's x range), 8 elsewhere; random: seeded, uniform in [0.5, 4]"""
    corners = np.asarray(node_pos)[np.asarray(elem_nodes)[:, :dim + 1]]
    if name == "bimaterial":
        x = corners[:, :, 0].mean(axis=1)
        px = np.asarray(node_pos)[:, 0]
        return np.where(x < 0.5 * (px.min() + px.max()), 1.0, 8.0)
    if name == "random":
        return np.random.default_rng(7).uniform(0.5, 4.0, len(elem_nodes))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def field(key, name):
    en, pos = mesh_tables(key)
    rho = density_field(name, en, pos, pos.shape[1])
    rho.setflags(write=False)
    return rho


def mass_matrix(dim, deg, elem_nodes, node_pos, rho=None, dof=None, n_dof=None):
    """M_rho as scipy CSR on interleaved displacement vectors; dof / n_dof: a DoF map (P^T M P)"""
    en = np.asarray(elem_nodes, dtype=np.int64)
    vol, _ = VL.geometry(node_pos, en[:, :dim + 1])
    rv = vol if rho is None else np.asarray(rho, dtype=np.float64) * vol
    m = VL.mass_coefficients(dim, deg)
    npe = en.shape[1]
    idx = en if dof is None else np.asarray(dof, dtype=np.int64)[en]
    n = len(node_pos) if n_dof is None else int(n_dof)
    rows = np.repeat(idx, npe, axis=1).ravel()
    cols = np.tile(idx, (1, npe)).ravel()
    vals = (rv[:, None, None] * m[None, :, :]).ravel()
    Ms = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    return sp.csr_matrix(sp.kron(Ms, sp.identity(dim)))


@functools.lru_cache(maxsize=None)
def M_rho(key, name=None):
    """M_rho of a modes_util mesh under field(key, name) (None: unit density)"""
    en, pos = mesh_tables(key)
    _, _, deg, _ = U.mesh_arrays(key)
    return mass_matrix(pos.shape[1], deg, en, pos, None if name is None else field(key, name))


def mass_properties(dim, elem_nodes, node_pos, rho=None):
    """{"mass", "com", "second_moment", "inertia"} from the closed forms; inertia = tr(S) I - S (3D), tr(S) (2D)"""
    P = np.asarray(node_pos, dtype=np.float64)[np.asarray(elem_nodes)[:, :dim + 1]]           # [nE, d + 1, d]
    vol, _ = VL.geometry(node_pos, np.asarray(elem_nodes)[:, :dim + 1])
    rv = vol if rho is None else np.asarray(rho, dtype=np.float64) * vol
    mass = rv.sum()
    com = (rv[:, None] * P.mean(axis=1)).sum(axis=0) / mass
    q = P - com
    sq = q.sum(axis=1)
    S = np.einsum("e,eab->ab", rv / ((dim + 1) * (dim + 2)), np.einsum("eka,ekb->eab", q, q) + np.einsum("ea,eb->eab", sq, sq))
    inertia = np.trace(S) * np.eye(3) - S if dim == 3 else float(np.trace(S))
    return {"mass": float(mass), "com": com, "second_moment": S, "inertia": inertia}


def rigid_mass_matrix(dim, props):
    """Z^T M Z for the rigid-body modes of modes_util.rigid_modes taken about the centre of mass: mass I on the translations, the inertia
    tensor (2D: the polar moment) on the rotations, no coupling"""
    nz = 6 if dim == 3 else 3
    R = np.zeros((nz, nz))
    R[:dim, :dim] = props["mass"] * np.eye(dim)
    R[dim:, dim:] = props["inertia"]
    return R


@functools.lru_cache(maxsize=None)
def clamped_truth(key, name):
    """(lam ascending, X columns, cond2(M_ff), eigh's own orthonormality defect) of (K, M_rho) clamped at modes_util.clamp_vars(key): dense on the
    small meshes, shift-invert eigsh about 0 on the mid mesh"""
    K, _ = U.pencil(key)
    Mr = M_rho(key, name)
    f = U.free_vars(key, U.clamp_vars(key))
    Kf, Mf = K[f][:, f], Mr[f][:, f]
    if key == U.MID:
        lam, X = U.shift_invert_eigsh(Kf, Mf, 0.0, 9)
        cond = U.cond_of_mass(Mf)
    else:
        lam, X = scipy.linalg.eigh(Kf.toarray(), Mf.toarray())
        cond = np.linalg.cond(Mf.toarray())
    defect = np.abs(X.T @ (Mf @ X) - np.eye(X.shape[1])).max()
    return lam, X, float(cond), float(defect)


@functools.lru_cache(maxsize=None)
def free_truth(key, name):
    """the free-free pencil (K, M_rho), dense: all eigenvalues ascending INCLUDING the 6 / 3 zeros"""
    K, _ = U.pencil(key)
    Mr = M_rho(key, name)
    lam, X = scipy.linalg.eigh(K.toarray(), Mr.toarray())
    cond = np.linalg.cond(Mr.toarray())
    defect = np.abs(X.T @ (Mr @ X) - np.eye(X.shape[1])).max()
    return lam, X, float(cond), float(defect)
