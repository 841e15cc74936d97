"""numpy twins of the modal stress recovery (docs/design/04_24_modal_stress.md), in float64 and np.longdouble, on the element sets of
tests/element_integrals_util.py and the von Mises value of tests/stress_measures_util.py. None of it touches the library under test.

    stress_sumsq_twin         sum over displacement planes, in plane order, of the squared corner stress components and of the squared von Mises value
                              (what k_modal_stress_sumsq accumulates)
    quadratic_stress_direct   sum_jk C_jk s_j^T A s_k from the per-column stress fields: the route WITHOUT the factor C = F F^T

In the precision of dtype from the vertex positions on: the barycentric gradients (closed-form inverse of the edge matrix), the shape-function
gradients at the interpolant nodes of element_integrals_util.strain_field, the symmetrised gradient, C : strain and the sums. An element set needs
its vertex positions for that: elem_set() below attaches them.

Flattened symmetric tensors carry TENSOR shear entries (2D xx yy xy, 3D xx yy zz yz xz xy), in which the von Mises form is
    3D: A = [[1, -1/2, -1/2], [-1/2, 1, -1/2], [-1/2, -1/2, 1]] (+) 3 I_3,    2D (plane stress): A = [[1, -1/2], [-1/2, 1]] (+) 3,
positive semi-definite (3D: the hydrostatic state is its null vector) with largest eigenvalue 3."""
import numpy as np

import element_integrals_util as U
from modal_random_util import cqc_twin
from oracle import meshfem_oracle as O

EPS = np.finfo(np.float64).eps


def elem_set(dim, deg, elem_nodes, verts, D, dof=None, n_dof=None):
    s = U.ElemSet(dim, deg, elem_nodes, verts, D, dof, n_dof)
    s.verts = np.asarray(verts, dtype=np.float64)
    return s


def vm_form(dim, dtype=np.float64):
    fl = dim * (dim + 1) // 2
    A = np.zeros((fl, fl), dtype=dtype)
    A[:dim, :dim] = dtype(-0.5)
    A[np.arange(dim), np.arange(dim)] = dtype(1)
    A[np.arange(dim, fl), np.arange(dim, fl)] = dtype(3)
    return A


def v2(flat):
    """The squared von Mises value as half a sum of squares (every term >= 0), in the precision of flat."""
    s = np.asarray(flat)
    half, three = s.dtype.type(0.5), s.dtype.type(3)
    if s.shape[-1] == 3:
        dd = s[..., 0] - s[..., 1]
        return half * (dd * dd + s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + three * (s[..., 2] * s[..., 2])
    d01, d12, d20 = s[..., 0] - s[..., 1], s[..., 1] - s[..., 2], s[..., 2] - s[..., 0]
    return half * (d01 * d01 + d12 * d12 + d20 * d20) + three * (s[..., 3] * s[..., 3] + s[..., 4] * s[..., 4] + s[..., 5] * s[..., 5])


def v2_size(flat_abs):
    """v2 with every difference replaced by the sum of the sizes: the natural size of v2's terms for entries of the sizes flat_abs >= 0."""
    s = np.asarray(flat_abs)
    half, three = s.dtype.type(0.5), s.dtype.type(3)
    if s.shape[-1] == 3:
        dd = s[..., 0] + s[..., 1]
        return half * (dd * dd + s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + three * (s[..., 2] * s[..., 2])
    d01, d12, d20 = s[..., 0] + s[..., 1], s[..., 1] + s[..., 2], s[..., 2] + s[..., 0]
    return half * (d01 * d01 + d12 * d12 + d20 * d20) + three * (s[..., 3] * s[..., 3] + s[..., 4] * s[..., 4] + s[..., 5] * s[..., 5])


def corner_gradients(s, dtype):
    """grad lambda_k of every element, [nE, N, N + 1] (element_integrals_util.ElemSet.gl's layout), in dtype: the columns of the inverse of the
    edge matrix E (rows v_k - v_0) by its adjugate, and minus their sum for k = 0."""
    N = s.N
    P = s.verts.astype(dtype)[s.en[:, :N + 1]]                   # [nE, N + 1, N]
    E = P[:, 1:] - P[:, :1]                                       # [nE, N, N]: row k - 1 = v_k - v_0
    if N == 2:
        det = E[:, 0, 0] * E[:, 1, 1] - E[:, 0, 1] * E[:, 1, 0]
        inv = np.stack([np.stack([E[:, 1, 1], -E[:, 0, 1]], axis=-1), np.stack([-E[:, 1, 0], E[:, 0, 0]], axis=-1)], axis=-2) / det[:, None, None]
    else:
        r0, r1, r2 = E[:, 0], E[:, 1], E[:, 2]
        c0, c1, c2 = np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)
        det = (r0 * c0).sum(axis=-1)
        inv = np.stack([c0, c1, c2], axis=-1) / det[:, None, None]          # column k = cofactors of row k
    gl = np.empty((len(s.en), N, N + 1), dtype=dtype)
    gl[:, :, 1:] = inv
    gl[:, :, 0] = -inv.sum(axis=-1)
    return gl


def gradphi_at_nodes(s, gl):
    """grad phi_i at the interpolant nodes of the strain (the centroid for degree 1, the corners for degree 2): [nE, nq, n, N] in gl's dtype
    (element_integrals_util.gradphi_at, which works in float64)."""
    dtype = gl.dtype.type
    nE, N, nv = gl.shape
    glT = np.transpose(gl, (0, 2, 1))
    if s.deg == 1:
        return glT[:, None].copy()
    pts = np.eye(nv, dtype=dtype)
    G = np.empty((nE, nv, O.num_nodes(s.K, 2), N), dtype=dtype)
    G[:, :, :nv] = glT[:, None] * (dtype(4) * pts - dtype(1))[None, :, :, None]
    for e in range(O.num_edges(s.K)):
        a, b = O.EDGE_START[e], O.EDGE_END[e]
        G[:, :, nv + e] = dtype(4) * (pts[None, :, b, None] * glT[:, None, a] + pts[None, :, a, None] * glT[:, None, b])
    return G


class Twin:
    """The element set's gradients and material in dtype, made once."""

    def __init__(self, s, dtype):
        self.s, self.dtype = s, dtype
        self.G = gradphi_at_nodes(s, corner_gradients(s, dtype))
        D = np.broadcast_to(s.D, (len(s.en),) + s.D.shape[1:]).astype(dtype)
        self.Dd = D * np.where(np.arange(D.shape[-1]) < s.N, dtype(1), dtype(2))[None, None, :]      # D times the shear doubling
        self.I, self.J = U.flat_pairs(s.N)

    def corner_field(self, u_nodes, stress, sizes=False):
        """[nE, nq, fl]: the strain (stress) of the nodal field u_nodes [nNode, N] at the interpolant nodes; sizes: the sums of the absolute terms"""
        dt = self.dtype
        u = np.asarray(u_nodes).astype(dt)[self.s.en]
        G, Dd = self.G, self.Dd
        if sizes:
            u, G, Dd = np.abs(u), np.abs(G), np.abs(Dd)
        g = np.einsum("eic,eqib->eqcb", u, G)
        eps = (dt(0.5) * (g + np.swapaxes(g, -1, -2)))[..., self.I, self.J]
        return np.einsum("erc,eqc->eqr", Dd, eps) if stress else eps


def stress_sumsq_twin(s, U_nodes, stress=True, dtype=np.float64, prefixes=None, sizes=False):
    """(vm [nE, nq], comp [nE, nq, fl]): the sums over the planes U_nodes [nPlanes, nNode, N], in plane order, of v2 and of the squared components
    of the corner strain / stress. prefixes: a list of plane counts -> {count: (vm, comp)} of the leading planes. sizes: the natural sizes of the
    entries instead (every term replaced by its absolute value)."""
    tw = s if isinstance(s, Twin) else Twin(s, dtype)
    nE, nq, fl = len(tw.s.en), tw.G.shape[1], len(tw.I)
    vm, comp = np.zeros((nE, nq), dtype=tw.dtype), np.zeros((nE, nq, fl), dtype=tw.dtype)
    out = {0: (vm.copy(), comp.copy())}
    for t, u in enumerate(U_nodes):
        f = tw.corner_field(u, stress, sizes)
        comp = comp + f * f
        vm = vm + (v2_size(f) if sizes else v2(f))
        out[t + 1] = (vm, comp)
    return {p: out[p] for p in prefixes} if prefixes is not None else (vm, comp)


def quadratic_stress_direct(s, X_nodes, C, stress=True, dtype=np.longdouble):
    """(vm2 [nE, nq], comp2 [nE, nq, fl]) = sum_jk C_jk s_j^T A s_k and sum_jk C_jk s_jc s_kc from the stress fields s_j of the columns X_nodes
    [nb, nNode, N]: the double sum as it stands, no factorisation."""
    tw = s if isinstance(s, Twin) else Twin(s, dtype)
    dt = tw.dtype
    S = np.array([tw.corner_field(x, stress) for x in X_nodes])              # [nb, nE, nq, fl]
    Cd = np.asarray(C).astype(dt)
    CS = np.einsum("jk,keqc->jeqc", Cd, S)
    comp2 = (S * CS).sum(axis=0)
    vm2 = np.einsum("jeqc,cd,jeqd->eq", S, vm_form(tw.s.N, dt), CS)
    return vm2, comp2


def worst_ratio(dev, ref_ld, ref_64, size):
    """(worst |dev - ref_ld| / size, worst |ref_64 - ref_ld| / size) over the entries with size > 0; entries of size 0 must be exact zeros."""
    dev, size = np.asarray(dev), np.asarray(size).astype(np.float64)
    pos = size > 0
    assert np.all(dev[~pos] == 0.0)
    if not pos.any():
        return 0.0, 0.0
    e = np.abs((dev - ref_ld).astype(np.float64))[pos] / size[pos]
    d = np.abs((np.asarray(ref_64) - ref_ld).astype(np.float64))[pos] / size[pos]
    return float(e.max()), float(d.max())


# ------------------------------------------------------------------------------------------------ shared by the reference test and the GPU tests
def matrices(lam, m, rng):
    """{name: C [m, m]}: diagonal, SRSS and CQC with random amplitudes, and a rank-deficient one."""
    a = rng.uniform(0.2, 1.0, m) / lam[:m]
    rho = np.asarray(cqc_twin(lam[:m], np.linspace(0.02, 0.07, m)), dtype=np.float64)
    rho = 0.5 * (rho + rho.T)
    G = rng.normal(size=(m, 3))
    return {"diagonal": np.diag(rng.uniform(0.1, 2.0, m)), "srss": np.diag(a * a), "cqc": np.outer(a, a) * rho, "rank-3": G @ G.T}


def factor_route(s, Xn, F, dtype):
    """the factor fields in dtype and their sums of squares"""
    planes = np.einsum("jt,jnd->tnd", np.asarray(F).astype(dtype), np.asarray(Xn).astype(dtype))
    return stress_sumsq_twin(s, planes, True, dtype)


def bars(s, Xn, F, truncation):
    """(long-double sums (vm2, comp2), bar on vm2, bar on comp2)"""
    v64, c64 = factor_route(s, Xn, F, np.float64)
    vld, cld = factor_route(s, Xn, F, np.longdouble)
    sj = np.array([Twin(s, np.float64).corner_field(x, True) for x in Xn])
    s2 = (sj * sj).sum(axis=0)                                     # [nE, nq, fl]: sum_j s_jc^2
    bar_v = 10.0 * float(np.abs((v64 - vld).astype(np.float64)).max()) + truncation * 3.0 * float(s2.sum(axis=-1).max())
    bar_c = 10.0 * float(np.abs((c64 - cld).astype(np.float64)).max()) + truncation * float(s2.max())
    return (vld, cld), bar_v, bar_c
