"""Expected values of the differential operators the device path provides (forced-degree-1 Laplacian / mass on a quadratic
mesh, the vector-valued mass matrix, divergence), pinned on the CPU oracle alone: the yardstick of
tests/test_gpu_differential_operators.py. FP64 tolerances are stated per assertion."""
import numpy as np
import pytest

from oracle import meshfem_oracle as O


def _mesh(dim, deg, seed=0):
    if dim == 3:
        V, T = O.grid_tet_mesh(3, 2, 2)
    else:
        V, Q = O.gen_grid_2d(4, 3)
        V, T = O.quad_tri_subdiv(V, Q)
        V = V[:, :2]
    rng = np.random.default_rng(seed)
    V = V + 0.08 * rng.standard_normal(V.shape)       # generic geometry, orientation preserved
    return O.FEMMesh(T, V, deg)


def vector_valued_expansion(n, i, j, v, N):
    """MassMatrix::construct_vector_valued (MassMatrix.hh:142-144) over summed scalar triplets: (N i + c, N j + c, v), c < N."""
    t = O.TripletMatrix(N * n, N * n)
    ii, jj, vv = [], [], []
    for a, b, w in zip(i, j, v):
        for c in range(N):
            ii.append(N * a + c); jj.append(N * b + c); vv.append(w)
    t.i, t.j, t.v = np.asarray(ii, np.int64), np.asarray(jj, np.int64), np.asarray(vv, np.float64)
    return t


def divergence_numpy(m, v):
    """differential_operators.cc:79-88 restated: out[n] = sum_{e containing n} v_e . int_e grad phi_n (degree 1: vol_e grad lambda_i)."""
    assert m.deg == 1
    vol, gl = m.embeddings_batch()                     # gl[e]: dim x (K + 1), column i = grad lambda_i
    out = np.zeros(m.num_nodes)
    for e, nodes in enumerate(m.elem_nodes):
        out[nodes] += vol[e] * (v[e] @ gl[e])
    return out


def l2sq_direct(m, u):
    vol, _ = m.embeddings_batch()
    pts, w = O.quadrature_rule(m.K, 2 * m.deg)
    Phi = np.array([O.shape_functions(m.deg, m.K, p) for p in pts])
    uq = np.einsum("qn,enc->eqc", Phi, u[m.elem_nodes])
    return float(np.einsum("q,e,eqc,eqc->", w, vol, uq, uq))


@pytest.mark.parametrize("dim", [2, 3])
def test_forced_p1_reference_is_the_linear_mesh_on_the_vertices(dim):
    m2 = _mesh(dim, 2)
    m1 = O.FEMMesh(m2.elems, m2.verts, 1)
    assert m1.num_nodes == len(m2.verts)
    assert np.array_equal(m1.elem_nodes, m2.elem_nodes[:, :dim + 1])       # vertex node index == vertex index (FEMMesh.inl:17-37)
    vol, gl = m1.embeddings_batch()
    n, K = m1.num_nodes, m1.K
    Lref, Mref = np.zeros((n, n)), np.zeros((n, n))
    for e, nodes in enumerate(m1.elem_nodes):
        Lref[np.ix_(nodes, nodes)] += gl[e].T @ gl[e] * vol[e]
        Mref[np.ix_(nodes, nodes)] += vol[e] * (np.ones((K + 1, K + 1)) + np.eye(K + 1)) / ((K + 1) * (K + 2))
    Lo = O.laplacian_triplets(m1).sum_repeated().to_scipy_full_from_upper().toarray()
    Mo = O.mass_triplets(m1).sum_repeated().to_scipy_full_from_upper().toarray()
    assert np.abs(Lo - Lref).max() < 1e-13 * np.abs(Lref).max()
    assert np.abs(Mo - Mref).max() < 1e-14 * np.abs(Mref).max()


@pytest.mark.parametrize("dim,deg", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_vector_valued_mass_is_the_l2_norm(dim, deg):
    m = _mesh(dim, deg)
    s = O.mass_triplets(m).sum_repeated()
    t = vector_valued_expansion(m.num_nodes, s.i, s.j, s.v, dim)
    assert t.nnz() == dim * s.nnz() and (t.i <= t.j).all()
    Mv = t.to_scipy_full_from_upper()
    rng = np.random.default_rng(0)
    for _ in range(8):
        u = rng.uniform(-1, 1, (m.num_nodes, dim))
        x = u.reshape(-1)
        l2 = x @ (Mv @ x)
        assert abs(l2 - l2sq_direct(m, u)) < 1e-13 * abs(l2)


@pytest.mark.parametrize("dim", [2, 3])
def test_divergence_is_the_transpose_of_volume_weighted_gradient(dim):
    m = _mesh(dim, 1)
    vol, _ = m.embeddings_batch()
    rng = np.random.default_rng(1)
    for _ in range(4):
        s, v = rng.standard_normal(m.num_nodes), rng.standard_normal((len(m.elems), dim))
        lhs = divergence_numpy(m, v) @ s
        rhs = float(np.einsum("e,ec,ec->", vol, v, O.grad_u_average(m, s)))
        assert abs(lhs - rhs) < 1e-12 * max(abs(lhs), abs(rhs))
