"""Brute-force numpy restatement of the field sampler (FieldSampler.hh of the reference; include/meshfem_hip.h "field sampler on the device"):
every point against every element / boundary element, no spatial index. V [nVert, dim], T [nElem, dim+1] vertex ids, P [nP, dim].
Tie rules as documented for the device: the lowest element index of all elements with min lambda >= -1e-12; the closest boundary element
under the total order (squared distance, index)."""
import numpy as np

CONTAIN_TOL = 1e-12
EDGE_START = [0, 1, 2, 0, 2, 1]          # Simplex.hh:43-44, the node order of the quadratic elements: node dim+1+j sits on edge (start, end)
EDGE_END = [1, 2, 0, 3, 3, 3]


def _inverse_edges(V, T):
    X0 = V[T[:, 0]]
    return X0, np.linalg.inv(V[T[:, 1:]] - X0[:, None, :])        # rows of the matrix: x_k - x_0


def bary_all(V, T, P):
    """barycentric coordinates of every point in every element: [nP, nElem, dim+1]"""
    X0, Minv = _inverse_edges(V, T)
    rest = np.einsum("pea,eak->pek", P[:, None, :] - X0[None], Minv)
    return np.concatenate([1.0 - rest.sum(axis=-1, keepdims=True), rest], axis=-1)


def bary_in(V, T, elems, P):
    """barycentric coordinates of point i in element elems[i]: [nP, dim+1]"""
    X0, Minv = _inverse_edges(V, T[elems])
    rest = np.einsum("pa,pak->pk", P - X0, Minv)
    return np.concatenate([1.0 - rest.sum(axis=-1, keepdims=True), rest], axis=-1)


def locate(V, T, P):
    """(I, B, minLam): the lowest-index element with min lambda >= -1e-12 (-1: none), its coordinates (NaN: none), min lambda [nP, nElem]"""
    lam = bary_all(V, T, P)
    mn = lam.min(axis=-1)
    inside = mn >= -CONTAIN_TOL
    I = np.where(inside.any(axis=1), inside.argmax(axis=1), -1)
    B = np.where((I >= 0)[:, None], lam[np.arange(len(P)), np.maximum(I, 0)], np.nan)
    return I, B, mn


def closest_on_segments(P, A, B):
    ab = B - A
    len2 = (ab * ab).sum(-1)
    t = np.where(len2 > 0, ((P - A) * ab).sum(-1) / np.where(len2 > 0, len2, 1.0), 0.0)
    return A + np.clip(t, 0.0, 1.0)[..., None] * ab


def closest_on_triangles(P, A, B, C):
    """closest point of triangle (A, B, C) to P by the vertex / edge / face region classification; all arrays broadcast to [..., 3]"""
    P, A, B, C = np.broadcast_arrays(P, A, B, C)
    ab, ac, ap, bp, cp = B - A, C - A, P - A, P - B, P - C
    dot = lambda x, y: (x * y).sum(-1)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    vals = [A, B, A + t_ab[..., None] * ab, C, A + t_ac[..., None] * ac, B + t_bc[..., None] * (C - B)]
    out = A + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]
    for cnd, val in reversed(list(zip(conds, vals))):          # the first condition that holds wins
        out = np.where(cnd[..., None], val, out)
    return out


def closest_on_simplices(V, S, P):
    """closest point of every simplex of S ([n, 2] segments in 2D, [n, 3] triangles in 3D) to every point: C [nP, n, dim], d2 [nP, n]"""
    Pb = P[:, None, :]
    if S.shape[1] == 2:
        C = closest_on_segments(Pb, V[S[:, 0]][None], V[S[:, 1]][None])
    else:
        C = closest_on_triangles(Pb, V[S[:, 0]][None], V[S[:, 1]][None], V[S[:, 2]][None])
    return C, ((Pb - C) ** 2).sum(-1)


def boundary_faces(T):
    """(faces [nBE, dim] vertex ids, parent [nBE]): the faces (edges in 2D) that belong to exactly one element"""
    nv = T.shape[1]
    faces = np.concatenate([np.delete(T, k, axis=1) for k in range(nv)])
    parent = np.tile(np.arange(len(T)), nv)
    key = np.sort(faces, axis=1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    keep = cnt[inv.reshape(-1)] == 1
    return faces[keep], parent[keep]


def closest_boundary(V, faces, P):
    """(index under the (d2, index) order, C [nP, dim], d2 [nP], all squared distances [nP, nBE])"""
    C, d2 = closest_on_simplices(V, faces, P)
    idx = d2.argmin(axis=1)                                      # argmin returns the first of equal minima: the lowest index
    r = np.arange(len(P))
    return idx, C[r, idx], d2[r, idx], d2


def dist2_to_elements(V, T, elems, P):
    """squared distance of point i to the (closed) element elems[i]: 0 inside, else the closest of its faces"""
    out = np.zeros(len(P))
    lam = bary_in(V, T, elems, P)
    for i in np.flatnonzero(lam.min(axis=1) < 0):
        f = np.stack([np.delete(T[elems[i]], k) for k in range(T.shape[1])])
        out[i] = closest_on_simplices(V, f, P[i:i + 1])[1].min()
    return out


def locate_full(V, T, P):
    """what mfh_locate returns, by brute force: (I, B, C, sqDist); outside points through the closest boundary face and its parent"""
    I, B, _ = locate(V, T, P)
    Cl, d2 = P.copy(), np.zeros(len(P))
    out = np.flatnonzero(I < 0)
    if len(out):
        faces, parent = boundary_faces(T)
        idx, C, dd, _ = closest_boundary(V, faces, P[out])
        I[out], Cl[out], d2[out] = parent[idx], C, dd
        B[out] = bary_in(V, T, parent[idx], C)
    return I, B, Cl, d2


def shape_functions(B, deg):
    """[nP, npe] values of the degree's shape functions at barycentric coordinates B [nP, dim+1]"""
    if deg == 1:
        return B.copy()
    ne = 3 if B.shape[1] == 3 else 6
    return np.concatenate([B * (2.0 * B - 1.0)] + [4.0 * B[:, [EDGE_START[j]]] * B[:, [EDGE_END[j]]] for j in range(ne)], axis=1)


def sample(elem_nodes, n_vert, deg, I, B, field):
    """MeshFieldSampler::sample at (I, B): the kind of field from its row count -- vertices, then elements, then nodes. elem_nodes [nElem, npe]
    (vertices first); rows with I = -1 are NaN."""
    f = np.asarray(field, dtype=np.float64)
    f2 = f.reshape(len(f), -1)
    ok = I >= 0
    Is = np.maximum(I, 0)
    nv = B.shape[1]
    if len(f) == n_vert:
        out = np.einsum("pk,pkc->pc", B, f2[elem_nodes[Is, :nv]])
    elif len(f) == len(elem_nodes):
        out = f2[Is].copy()
    elif len(f) == elem_nodes.max() + 1:
        out = np.einsum("pk,pkc->pc", shape_functions(B, deg), f2[elem_nodes[Is]])
    else:
        raise ValueError("Invalid fieldValues size")
    out[~ok] = np.nan
    return out.reshape((len(I),) + f.shape[1:])


def closest_node(elem_nodes, node_pos, deg, I, B, P):
    """(node, squared distance to P, lead of the largest shape function over the second): argmax takes the lowest local index on ties"""
    N = shape_functions(B, deg)
    j = N.argmax(axis=1)
    node = elem_nodes[np.maximum(I, 0), j]
    srt = np.sort(N, axis=1)
    return node, ((node_pos[node] - P) ** 2).sum(-1), srt[:, -1] - srt[:, -2]
