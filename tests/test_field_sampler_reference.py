"""The numpy restatement of the field sampler (tests/field_sampler_util.py) on closed forms; no GPU. The device kernels are compared with
this restatement in tests/test_gpu_field_sampler.py."""
import numpy as np
import pytest

import field_sampler_util as R

CASES = [(2, 1), (2, 2), (3, 1), (3, 2)]


def _mesh(dim, deg):
    """(V, T, elem_nodes, node positions) of a small perturbed mesh in the library's node numbering (host-only context: no device)"""
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(3, 2, 2) if dim == 3 else grid.grid_tri_mesh(4, 3)
    V = V + 0.05 * np.random.default_rng(1).standard_normal(V.shape)
    c = M.Context(-1)
    c.mesh_build(T, V, deg)
    en, npos = c.elem_nodes(), c.node_positions()
    c.close()
    return np.ascontiguousarray(V), np.ascontiguousarray(T), en, npos


def _interior_points(V, T, n, rng):
    e = rng.integers(0, len(T), n)
    w = rng.dirichlet(np.ones(T.shape[1]), n)
    return e, np.einsum("pk,pka->pa", w, V[T[e]])


def _poly(X, deg, ncomp, rng):
    """ncomp polynomials of total degree <= deg at the points X"""
    d = X.shape[1]
    terms = [np.ones(len(X))] + [X[:, a] for a in range(d)]
    if deg == 2:
        terms += [X[:, a] * X[:, b] for a in range(d) for b in range(a, d)]
    coef = rng.standard_normal((len(terms), ncomp))
    return lambda Y: np.stack([np.ones(len(Y))] + [Y[:, a] for a in range(d)] +
                              ([Y[:, a] * Y[:, b] for a in range(d) for b in range(a, d)] if deg == 2 else []), axis=1) @ coef


@pytest.mark.parametrize("dim,deg", CASES)
def test_polynomials_are_reproduced_at_interior_points(dim, deg):
    V, T, en, npos = _mesh(dim, deg)
    rng = np.random.default_rng(5)
    _, P = _interior_points(V, T, 200, rng)
    I, B, _ = R.locate(V, T, P)
    assert np.all(I >= 0)
    q = _poly(npos, deg, 3, rng)
    field = q(npos)                                             # one row per node
    got = R.sample(en, len(V), deg, I, B, field)
    assert np.abs(got - q(P)).max() <= 1e-13 * np.abs(field).max()
    q1 = _poly(V, 1, 2, rng)                                     # per-vertex fields are linear whatever the degree
    assert np.abs(R.sample(en, len(V), deg, I, B, q1(V)) - q1(P)).max() <= 1e-13 * np.abs(q1(V)).max()
    per_elem = rng.standard_normal((len(T), 2))
    assert np.array_equal(R.sample(en, len(V), deg, I, B, per_elem), per_elem[I])


@pytest.mark.parametrize("dim", [2, 3])
def test_barycentric_coordinates_sum_to_one_and_reproduce_the_point(dim):
    V, T, _, _ = _mesh(dim, 1)
    rng = np.random.default_rng(6)
    e, P = _interior_points(V, T, 100, rng)
    lam = R.bary_all(V, T, P)
    assert np.abs(lam.sum(-1) - 1.0).max() <= 1e-13
    assert np.abs(np.einsum("pek,eka->pea", lam, V[T]) - P[:, None, :]).max() <= 1e-12
    I, B, _ = R.locate(V, T, P)
    assert np.array_equal(I, e) or np.all(R.bary_in(V, T, I, P).min(axis=1) >= -R.CONTAIN_TOL)
    assert np.abs(B - R.bary_in(V, T, I, P)).max() <= 1e-13


def test_lowest_index_wins_on_a_shared_edge():
    V = np.array([[0.0, 0], [1, 0], [1, 1], [0, 1]])
    T = np.array([[0, 1, 2], [0, 2, 3]])
    I, B, _ = R.locate(V, T, np.array([[0.5, 0.5], [0.25, 0.75], [2.0, 2.0]]))
    assert I.tolist() == [0, 1, -1] and np.all(np.isnan(B[2]))


def test_closest_points_to_the_unit_square():
    from meshfem_amd import grid
    V, T = grid.grid_tri_mesh(3, 3, [0, 0], [1, 1])
    P = np.array([[1.5, 0.3], [-0.2, 0.6], [0.4, 1.7], [0.4, -0.1], [1.5, 1.25], [-1.0, -2.0], [-0.5, 1.5], [2.0, -0.5]])   # 4 edge, 4 corner regions
    I, B, C, d2 = R.locate_full(V, T, P)
    want = np.clip(P, 0.0, 1.0)
    assert np.abs(C - want).max() <= 1e-15 and np.abs(d2 - ((P - want) ** 2).sum(1)).max() <= 1e-15
    assert np.abs(np.einsum("pk,pka->pa", B, V[T[I]]) - want).max() <= 1e-14


def test_closest_points_to_the_unit_cube():
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(2, 2, 2, [0, 0, 0], [1, 1, 1])
    P = np.array([[1.5, 0.3, 0.6], [0.2, -0.4, 0.7], [0.3, 0.6, 2.0],            # face regions
                  [1.5, 1.5, 0.4], [-0.5, 0.3, -0.25], [0.6, 2.0, 1.5],           # edge regions
                  [1.5, 1.25, 2.0], [-1.0, -1.0, -1.0], [2.0, -0.5, 1.5]])        # corner regions
    I, B, C, d2 = R.locate_full(V, T, P)
    want = np.clip(P, 0.0, 1.0)
    assert np.abs(C - want).max() <= 1e-15 and np.abs(d2 - ((P - want) ** 2).sum(1)).max() <= 1e-15
    assert np.abs(np.einsum("pk,pka->pa", B, V[T[I]]) - want).max() <= 1e-14
    assert np.all(R.dist2_to_elements(V, T, I, P) <= d2 + 1e-15)


def test_closest_node_takes_the_largest_shape_function():
    V, T, en, npos = _mesh(2, 2)
    B = np.array([[0.8, 0.1, 0.1], [0.45, 0.45, 0.1], [1 / 3, 1 / 3, 1 / 3]])
    I = np.array([0, 1, 2])
    P = np.einsum("pk,pka->pa", B, V[T[I]])
    node, d2, lead = R.closest_node(en, npos, 2, I, B, P)
    assert node[0] == en[0, 0] and node[1] == en[1, 3]              # a vertex; the node of edge (0, 1)
    assert lead[2] <= 1e-15 and node[2] == en[2, 3]                 # the three edge functions tie at the centroid: lowest local index
    assert np.abs(d2 - ((npos[node] - P) ** 2).sum(1)).max() == 0
