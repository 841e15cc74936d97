"""Shared helpers of the prestressed-vibration tests (mfh_modes_prestressed, mfh_tangent_apply; docs/design/04_18_prestressed_modes.md): the dense
truth eigh((K + s Kg)_ff, M_ff) on the column fixtures of buckling_util -- K from the CPU oracle, Kg from buckling_util's numpy restatement, M from
density_util's -- under unit axial compression, the critical factor of each column, and the componentwise rounding bounds of the pair product
yA + s Kg x, rho M x. Every matrix and every spectrum is computed once per process (functools.lru_cache), handed out read-only."""
import functools

import numpy as np
import scipy.linalg

import buckling_util as B
import density_util as D
import modes_util as U

EPS = U.EPS
COLUMNS = B.COLUMNS
FACTORS = (-1.0, 0.5, 0.9, 1.1)          # multiples of the critical factor the GPU tests solve at


def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def deg_of(key):
    return B.mesh_arrays(key)[2]


@functools.lru_cache(maxsize=None)
def mass(key):
    """M at unit density, scipy CSR on interleaved displacement vectors"""
    en, pos = B.mesh_tables(key)
    return D.mass_matrix(pos.shape[1], deg_of(key), en, pos)


@functools.lru_cache(maxsize=None)
def free_blocks(key):
    """(K_ff, Kg_ff under unit axial compression, M_ff) dense, clamped at buckling_util.clamp_vars"""
    f = B.free_vars(key)
    Kf = B.stiffness(key)[f][:, f].toarray()
    Gf = B.Kg_of(key, B.axial_compression(key))[f][:, f].toarray()
    Mf = mass(key)[f][:, f].toarray()
    return _readonly(Kf, Gf, Mf)


@functools.lru_cache(maxsize=None)
def critical_factor(key):
    """the smallest load factor -1 / mu_min of Kg x = mu K x (buckling_util.column_truth)"""
    mu = B.column_truth(key)[0]
    assert mu[0] < 0
    return float(-1.0 / mu[0])


@functools.lru_cache(maxsize=None)
def cond_of_mass(key):
    return float(np.linalg.cond(free_blocks(key)[2]))


def dense_spectrum(Kf, Gf, Mf, s):
    """(lam ascending, X columns, eigh's own M-orthonormality defect) of (K + s Kg) x = lam M x"""
    lam, X = scipy.linalg.eigh(Kf + s * Gf, Mf)
    defect = np.abs(X.T @ (Mf @ X) - np.eye(X.shape[1])).max()
    return lam, X, float(defect)


@functools.lru_cache(maxsize=None)
def truth(key, ratio):
    """dense_spectrum at s = ratio x the critical factor under unit axial compression"""
    Kf, Gf, Mf = free_blocks(key)
    lam, X, defect = dense_spectrum(Kf, Gf, Mf, ratio * critical_factor(key))
    _readonly(lam, X)
    return lam, X, defect


def relative_gaps(lam, count=6):
    """(lam_{i+1} - lam_i) / max(|lam_i|, |lam_{i+1}|) among the first `count` eigenvalues"""
    l = np.asarray(lam[:count])
    return np.diff(l) / np.maximum(np.abs(l[:-1]), np.abs(l[1:]))


def host_residuals(A, Mm, lam, X):
    """||A x - lam M x||_2 / (|lam| ||M x||_2) per row of X"""
    AX, MX = A @ X.T, Mm @ X.T
    return np.linalg.norm(AX - MX * lam[None, :], axis=0) / (np.abs(lam) * np.linalg.norm(MX, axis=0))


# ------------------------------------------------------------------------------------------------ rounding bounds of the pair product
def mass_product_bound(dim, deg, elem_nodes, node_pos, rho, x, dof=None, n_dof=None):
    """The analogue of buckling_util.product_bound for y = M x: (N_r + ROUNDINGS_PER_CONTRIBUTION) eps sum_j |M|_rj |x_j| per row r, |M| with every
    (element, i, j) summand taken by modulus (quadratic elements have negative coefficients) and the volume by its own componentwise perturbation
    bound. The chain of a mass contribution (volume, coefficient, density) is shorter than that of a Kg contribution, so the same allowance holds."""
    import math
    import volume_loads_util as VL
    en = np.asarray(elem_nodes, dtype=np.int64)
    P = np.asarray(node_pos, dtype=np.float64)[en[:, :dim + 1]]
    nE, nv, _ = P.shape
    A = np.concatenate([np.ones((nE, 1, nv)), np.swapaxes(P, 1, 2)], axis=1)
    Ai = np.linalg.inv(A)
    vol = np.abs(np.linalg.det(A)) / math.factorial(dim)
    vol_abs = vol * np.einsum("eij,eji->e", np.abs(A), np.abs(Ai)) / nv
    rv = vol_abs if rho is None else np.abs(np.asarray(rho, dtype=np.float64)) * vol_abs
    Me = rv[:, None, None] * np.abs(np.asarray(VL.mass_coefficients(dim, deg)))[None, :, :]
    idx = en if dof is None else np.asarray(dof, dtype=np.int64)[en]
    n = len(node_pos) if n_dof is None else int(n_dof)
    Mabs = B._scalar_to_sparse(Me, idx, n)
    count = np.asarray(B._scalar_to_sparse(np.ones_like(Me), idx, n).sum(axis=1)).ravel()
    xa = np.abs(np.asarray(x, dtype=np.float64)).reshape(n, -1)
    return ((count[:, None] + B.ROUNDINGS_PER_CONTRIBUTION) * EPS * (Mabs @ xa)).reshape(np.shape(x))


def pair_bounds(s, rho, yA0, ref_G, ref_M, bound_G, bound_M):
    """Bars of the two outputs of the pair product from the bars of the plain products Kg x and M x (ref_*: their values in numpy):
      yA = yA0 + s (Kg x): |s| bound_G, the rounding of the scaling (eps |s Kg x|) and of the sum (eps |yA0 + s Kg x| <= eps (|yA0| + |s Kg x|))
      yB = rho (M x):      |rho| bound_M and the rounding of the scaling
    (the second-order terms are covered by the factor 2 on the two single roundings)"""
    sg = np.abs(s) * np.abs(ref_G)
    bar_A = np.abs(s) * bound_G + 2 * EPS * (sg + np.abs(yA0))
    bar_B = np.abs(rho) * bound_M + 2 * EPS * np.abs(rho) * np.abs(ref_M)
    return bar_A, bar_B
