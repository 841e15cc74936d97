"""A plain reference of the preconditioned conjugate gradients the solver runs, iterate by iterate: x_0 = 0, the text-book (classic)
recurrences, and the same walk in the Chronopoulos-Gear form as the header comment of the kernels states it
(meshfem_amd/csrc/mfh_kernels_solver.hip: "Chronopoulos-Gear PCG"). The operator and the preconditioner are callables; the Dirichlet
lift b = mask(f - K ubar) and u = x + ubar are part of the reference, as they are part of mfh_solve. Dot products are accumulated in
extended precision (np.longdouble) unless asked otherwise; the vectors are FP64, or longdouble throughout with dtype=np.longdouble (the
callables must then accept and return longdouble vectors: csr_apply and block_jacobi_apply do).

Shared by tests/test_pcg_iterates_reference.py (CPU: the reference against a dense direct solve and against itself) and
tests/test_gpu_pcg_iterates.py (the four PCG loops of the library against it)."""
import types

import numpy as np
import scipy.sparse as sp


# ------------------------------------------------------------------------------------------------ the problems of both test files
def mesh(dim, size=None):
    """3D: 4 x 3 x 3 cells (1 509 P2 nodes: three workgroups of the pair-per-lane kernels, the last with a partial wave), 2D: 20 x 16
    quads; interior vertices moved by up to 4 % (element_integrals_util.perturbed)."""
    from meshfem_amd import grid
    from element_integrals_util import perturbed
    V, T = grid.grid_tet_mesh(*(size or (4, 3, 3))) if dim == 3 else grid.grid_tri_mesh(*(size or (20, 16)))
    return perturbed(V, 0.04), np.asarray(T)


def iso_field(dim, n_elem):
    """The isotropic field of test_gpu_preconditioner_maps._setup (E varies by 6x): (E, nu, D of every element)."""
    from oracle import meshfem_oracle as O
    rng = np.random.default_rng(21)
    E, nu = rng.uniform(50.0, 300.0, n_elem), rng.uniform(0.1, 0.4, n_elem)
    return E, nu, np.stack([O.ElasticityTensor.isotropic(dim, a, b).D for a, b in zip(E, nu)])


def oracle_K(dim, deg, elem_nodes, V, D, n_dof, dof=None):
    """The oracle's K mirrored to the full symmetric matrix, CSR (as test_gpu_operator_maps._oracle_K)."""
    from oracle import c_oracle as CO
    Ap, Ai, Ax, _ = CO.assemble_csc(dim, deg, elem_nodes, V, D, n_dof, dof)
    n = dim * n_dof
    U = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
    return (U + U.T - sp.diags(U.diagonal())).tocsr()


def oracle_laplacian(T, V, deg):
    """(the oracle's scalar Laplacian, full symmetric CSR; its FEMMesh)"""
    from oracle import meshfem_oracle as O
    m = O.FEMMesh(np.asarray(T), np.asarray(V, dtype=np.float64), deg)
    return O.laplacian_triplets(m).sum_repeated().to_scipy_full_from_upper().tocsr(), m


# ------------------------------------------------------------------------------------------------ the reference
def dot_longdouble(a, b):
    return np.dot(np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble))


def dot_fp64(a, b):
    return np.dot(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


def csr_apply(K, dtype=np.float64):
    """apply_K of a sparse matrix for FP64 or longdouble vectors (scipy has no extended-precision product: the rows are summed here)."""
    K = sp.csr_matrix(K)
    if dtype == np.float64:
        return lambda v: K @ v
    K.sort_indices()
    data, idx, starts = K.data.astype(dtype), K.indices, K.indptr[:-1]
    assert np.all(np.diff(K.indptr) > 0), "an empty row"
    return lambda v: np.add.reduceat(data * np.asarray(v, dtype=dtype)[idx], starts)


def _setup(apply_K, f, fixed, ubar, dtype):
    fixed = np.asarray(fixed, dtype=bool)
    f = np.asarray(f, dtype=dtype)
    ub = np.zeros(len(f), dtype=dtype)
    if ubar is not None:
        ub[fixed] = np.asarray(ubar, dtype=dtype)[fixed]
    b = f - apply_K(ub) if np.any(ub != 0) else f.copy()
    b[fixed] = 0
    return fixed, ub, b


def _result(X, rr, bb, ub, rtol):
    res = np.array([float(np.sqrt(v / bb)) if bb > 0 else 0.0 for v in rr])
    k_stop = None
    if rtol is not None:
        hit = np.nonzero(res <= rtol)[0]
        k_stop = int(hit[0]) if len(hit) else None
    return types.SimpleNamespace(u=[np.asarray(x + ub, dtype=np.float64) for x in X], res=res, k_stop=k_stop, bb=float(bb))


def pcg_classic(apply_K, apply_M, f, fixed, ubar=None, iters=12, rtol=None, dot=dot_longdouble, dtype=np.float64, stop=False):
    """u[k] = x_k + ubar and res[k] = |r_k| / |b| for k = 0 .. iters; k_stop: the first k with res[k] <= rtol (None: not within iters).
    stop: end the walk at k_stop (the lists are then that short).
    fixed: boolean mask of the fixed rows; ubar: their values (any vector of full length, read on the fixed rows; None: zero)."""
    fixed, ub, b = _setup(apply_K, f, fixed, ubar, dtype)

    def K(v):
        y = np.asarray(apply_K(v), dtype=dtype)
        y[fixed] = 0
        return y

    def M(v):
        z = np.asarray(apply_M(v), dtype=dtype)
        z[fixed] = 0
        return z
    bb = dot(b, b)
    x = np.zeros(len(b), dtype=dtype)
    X, rr = [x.copy()], [bb]
    if not bb > 0:
        return _result(X * (iters + 1), [bb] * (iters + 1), bb, ub, rtol)
    r = b.copy()
    z = M(r)
    p = z.copy()
    rz = dot(r, z)
    for _ in range(iters):
        Ap = K(p)
        alpha = dtype(rz / dot(p, Ap))
        x = x + alpha * p
        r = r - alpha * Ap
        z = M(r)
        rz_new = dot(r, z)
        beta = dtype(rz_new / rz)
        p = z + beta * p
        rz = rz_new
        X.append(x.copy())
        rr.append(dot(r, r))
        if stop and rtol is not None and rr[-1] <= rtol * rtol * bb:
            break
    return _result(X, rr, bb, ub, rtol)


def pcg_chronopoulos_gear(apply_K, apply_M, f, fixed, ubar=None, iters=12, rtol=None, dot=dot_longdouble, dtype=np.float64):
    """The same iterates by the recurrences of the kernel header: u = M^-1 r, w = K u, gamma = (r, u), delta = (w, u);
    beta = gamma_it / gamma_it-1, alpha = gamma_it / (delta_it - beta gamma_it / alpha_it-1);
    p = u + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s."""
    fixed, ub, b = _setup(apply_K, f, fixed, ubar, dtype)

    def K(v):
        y = np.asarray(apply_K(v), dtype=dtype)
        y[fixed] = 0
        return y

    def M(v):
        z = np.asarray(apply_M(v), dtype=dtype)
        z[fixed] = 0
        return z
    bb = dot(b, b)
    x = np.zeros(len(b), dtype=dtype)
    X, rr = [x.copy()], [bb]
    if not bb > 0:
        return _result(X * (iters + 1), [bb] * (iters + 1), bb, ub, rtol)
    r = b.copy()
    p = np.zeros_like(x)
    s = np.zeros_like(x)
    u = M(r)
    w = K(u)
    gamma, delta = dot(r, u), dot(w, u)
    gamma_prev = alpha_prev = None
    for it in range(iters):
        if it == 0:
            beta, alpha = dtype(0), dtype(gamma / delta)
        else:
            beta = dtype(gamma / gamma_prev)
            alpha = dtype(gamma / (delta - beta * gamma / alpha_prev))
        p = u + beta * p
        s = w + beta * s
        x = x + alpha * p
        r = r - alpha * s
        u = M(r)
        gamma_prev, alpha_prev = gamma, alpha
        gamma = dot(r, u)
        w = K(u)
        delta = dot(w, u)
        X.append(x.copy())
        rr.append(dot(r, r))
    return _result(X, rr, bb, ub, rtol)


def exact_stop(res):
    """(k*, rtol): k* the first iteration whose residual lies at least 10 % below every earlier one, rtol the geometric mean of res[k*] and
    the smallest earlier residual -- a threshold that rounding cannot move to a neighbouring iteration."""
    for k in range(1, len(res)):
        best = min(res[:k])
        if res[k] <= 0.9 * best:
            return k, float(np.sqrt(res[k] * best))
    raise AssertionError("no iteration falls 10 %% below its predecessors: %s" % (res,))


def block_jacobi_blocks(K, bs, fixed):
    """The diagonal bs x bs blocks of K [n_dof, bs, bs], the fixed components decoupled (their rows and columns replaced by identity)."""
    n = K.shape[0]
    K = sp.csr_matrix(K)
    base = np.arange(0, n, bs)
    B = np.empty((len(base), bs, bs))
    for a in range(bs):
        for b in range(bs):
            B[:, a, b] = np.asarray(K[base + a, base + b]).ravel()
    fx = np.asarray(fixed, dtype=bool).reshape(-1, bs)
    q, a = np.nonzero(fx)
    B[q, a, :] = 0.0
    B[q, :, a] = 0.0
    B[q, a, a] = 1.0
    return B


def block_jacobi_apply(K, bs, fixed):
    """apply_M of the block-Jacobi preconditioner: z = B_q^-1 r_q per DoF block, zero on the fixed rows."""
    Binv = np.linalg.inv(block_jacobi_blocks(K, bs, fixed))
    free = ~np.asarray(fixed, dtype=bool)

    def apply(r):
        r = np.asarray(r)
        z = np.einsum("qab,qb->qa", Binv.astype(r.dtype), r.reshape(-1, bs)).ravel()
        return z * free
    return apply


def two_eigenvector_rhs(K, bs, fixed, sigmas=(0.5, 1.5)):
    """b = D (v_i + 0.7 v_j) on the free rows (zero on the fixed ones) for two generalized eigenvectors K v = lambda D v of the free rows,
    D the block-Jacobi blocks: PCG with M = D^-1 from x_0 = 0 ends at exactly the second iteration (the Krylov space of M^-1 K and
    M^-1 b is two-dimensional). The eigenvectors are those nearest to the two shifts (the spectrum of D^-1 K fills (0, 2) and beyond),
    by shift-and-invert Lanczos on the sparse matrices, converged to working precision."""
    import scipy.sparse.linalg as spla
    fixed = np.asarray(fixed, dtype=bool)
    free = np.nonzero(~fixed)[0]
    Kff = sp.csc_matrix(sp.csr_matrix(K)[free][:, free])
    D = sp.block_diag(list(block_jacobi_blocks(K, bs, fixed)), format="csc")[free][:, free]
    pairs = [spla.eigsh(Kff, k=1, M=D, sigma=s, which="LM", tol=0, v0=np.ones(len(free))) for s in sigmas]
    (wi, vi), (wj, vj) = pairs
    assert abs(wi[0] - wj[0]) > 0.1 * abs(wj[0]), (wi, wj)
    b = np.zeros(K.shape[0])
    b[free] = D @ (vi[:, 0] + 0.7 * vj[:, 0])
    return b
