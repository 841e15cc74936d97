"""The differential operators on the device against the CPU oracle: the vector-valued mass matrix (OP_MASS_VECTOR, one stored
value per block, k_spmv_kron), the forced-degree-1 view of a quadratic context, the lumped mass matrix (k_row_sums), divergence and
gradient. Tolerances are those tests/test_scalar_operators.py holds the full-degree operators to: 1e-13 max|A_ref| for matrices,
1e-12 max|A_ref x| for applications, 1e-14 max for lumped diagonals."""
import numpy as np
import pytest

from oracle import meshfem_oracle as O

pytestmark = pytest.mark.gpu

CASES = [(2, 1), (2, 2), (3, 1), (3, 2)]


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


def _expand(s, N):
    """MassMatrix::construct_vector_valued over summed scalar upper triplets, in the column-major (dumpBinary) order."""
    i = (N * s.i[:, None] + np.arange(N)[None, :]).reshape(-1)
    j = (N * s.j[:, None] + np.arange(N)[None, :]).reshape(-1)
    v = np.repeat(s.v, N)
    order = np.lexsort((i, j))
    return i[order], j[order], v[order]


def _scalar_pattern(m):
    """The upper-triangle entries MassMatrix::construct holds after sumRepeated, in its column-major order, computed from the mesh alone:
    the node pairs that share an element, minus the pairs whose integral vanishes analytically. On quadratic TRIANGLES those are a vertex
    and the two edge nodes next to it (reference table x 180 / area: vertex row 6 -1 -1 | 0 -4 0); quadratic tets and linear elements have
    none. There the reference's quadrature (MassMatrix.hh:69-74) and the oracle hold rounding noise (<= 2e-19 against max 0.12 here) that
    sumRepeated keeps or drops as it happens to cancel; the device's exact table gives 0.0, which the export prunes (pruneTol = 0)."""
    K, n = m.K, m.nodes_per_elem
    pairs = set()
    for nodes in m.elem_nodes:
        for a in range(n):
            for b in range(n):
                if m.deg == 2 and K == 2:
                    v, e = (a, b) if a < 3 <= b else ((b, a) if b < 3 <= a else (None, None))
                    if v is not None and v in ((e - 3) % 3, (e - 3 + 1) % 3):      # edge node 3 + k lies between vertices k and k + 1
                        continue
                i, j = int(nodes[a]), int(nodes[b])
                if i <= j:
                    pairs.add((j, i))
    cols_rows = np.array(sorted(pairs), dtype=np.int64)
    return cols_rows[:, 1], cols_rows[:, 0]


def _same_triplets(m, s, N, i, j, v, tol=1e-13):
    """Exported triplets (i, j, v) of the N-fold expansion against the expected pattern, entry for entry and in order, and against the
    oracle's summed scalar triplets `s` for the values (tol max|ref|); what the oracle holds outside the pattern must be noise."""
    pi, pj = _scalar_pattern(m)
    ei = (N * pi[:, None] + np.arange(N)[None, :]).reshape(-1)
    ej = (N * pj[:, None] + np.arange(N)[None, :]).reshape(-1)
    order = np.lexsort((ei, ej))
    ei, ej = ei[order], ej[order]
    assert len(v) == N * len(pi)                                        # nnz == N nnz_scalar
    assert np.array_equal(np.asarray(i).astype(np.int64), ei) and np.array_equal(np.asarray(j).astype(np.int64), ej)
    S = s.to_scipy().tocsr()
    cut = tol * np.abs(s.v).max()
    ref = np.asarray(S[ei // N, ej // N]).reshape(-1)
    assert np.abs(v - ref).max() < cut
    inside = set(zip(pi.tolist(), pj.tolist()))
    outside = np.array([abs(w) for a, b, w in zip(s.i.tolist(), s.j.tolist(), s.v.tolist()) if (a, b) not in inside])
    assert outside.size == 0 or outside.max() < 1e-3 * cut               # rounding noise of an integral that is zero
    return outside.size


def _full(n, i, j, v):
    import scipy.sparse as sp
    U = sp.coo_matrix((v, (i, j)), shape=(n, n)).tocsr()
    return U + sp.triu(U, 1).T


def _l2sq_direct(m, u):
    vol, _ = m.embeddings_batch()
    pts, w = O.quadrature_rule(m.K, 2 * m.deg)
    Phi = np.array([O.shape_functions(m.deg, m.K, p) for p in pts])
    uq = np.einsum("qn,enc->eqc", Phi, u[m.elem_nodes])
    return float(np.einsum("q,e,eqc,eqc->", w, vol, uq, uq))


def _divergence_numpy(m, v):
    vol, gl = m.embeddings_batch()
    out = np.zeros(m.num_nodes)
    for e, nodes in enumerate(m.elem_nodes):
        out[nodes] += vol[e] * (v[e] @ gl[e])
    return out


def _ctx(m, deg, op):
    import meshfem_amd as M
    c = M.Context(0)
    c.mesh_build(m.elems, m.verts, deg)
    assert np.array_equal(c.elem_nodes(), m.elem_nodes)
    c.set_operator(op)
    return c


@pytest.mark.parametrize("dim,deg", CASES)
def test_vector_mass_export(dim, deg):
    import meshfem_amd as M
    m = _mesh(dim, deg, seed=3)
    s = O.mass_triplets(m).sum_repeated()
    ri, rj, rv = _expand(s, dim)
    c = _ctx(m, deg, M.OP_MASS_VECTOR)
    assert c.bs == dim
    c.assemble()
    i, j, v = c.export_upper_triplets()
    noise = _same_triplets(m, s, dim, i, j, v)
    if not (dim == 2 and deg == 2):
        # no vanishing integrals: the reference expansion itself, entry for entry
        assert noise == 0 and len(v) == dim * s.nnz()
        assert np.array_equal(i.astype(np.int64), ri) and np.array_equal(j.astype(np.int64), rj)
        assert np.abs(v - rv).max() < 1e-13 * np.abs(rv).max()
    else:
        # quadratic triangles: 478 scalar entries remain of the 588 node pairs that share an element (110 vertex / adjacent-edge-node
        # pairs vanish), each exported once per component
        assert len(v) == 2 * 478
    # the block matrix itself: m_ij I
    A = c.export_scipy().toarray()
    A_ref = _full(dim * m.num_nodes, ri, rj, rv).toarray()
    assert np.abs(A - A_ref).max() < 1e-13 * np.abs(A_ref).max()


@pytest.mark.parametrize("dim,deg", CASES)
def test_vector_mass_application(dim, deg):
    import meshfem_amd as M
    m = _mesh(dim, deg, seed=3)
    n = m.num_nodes
    A_ref = _full(dim * n, *_expand(O.mass_triplets(m).sum_repeated(), dim))
    c = _ctx(m, deg, M.OP_MASS_VECTOR)
    c.set_option("deterministic", 1)
    rng = np.random.default_rng(5)
    x = rng.standard_normal(dim * n)
    y = c.apply_K(x)
    ref = A_ref @ x
    assert np.abs(y - ref).max() < 1e-12 * np.abs(ref).max()
    assert np.array_equal(c.apply_K(x), y)                       # no atomics in k_spmv_kron
    u = rng.uniform(-1, 1, (n, dim))
    l2 = u.reshape(-1) @ c.apply_K(u.reshape(-1))
    assert abs(l2 - _l2sq_direct(m, u)) < 1e-13 * abs(l2)        # the reference's test_mass.cc "L2 Norm Validation"


@pytest.mark.parametrize("dim,deg", CASES)
def test_vector_mass_solve(dim, deg):
    import meshfem_amd as M
    m = _mesh(dim, deg, seed=3)
    n = m.num_nodes
    c = _ctx(m, deg, M.OP_MASS_VECTOR)
    c.set_preconditioner(M.PRECOND_JACOBI)
    rng = np.random.default_rng(7)
    u0 = rng.standard_normal(dim * n)
    f = c.apply_K(u0)
    u = c.solve(f, rtol=1e-12, maxit=5000)
    assert c.last_info["converged"] == 1
    err = np.abs(u - u0).max() / np.abs(u0).max()
    assert err <= 1e-9, "|u - u0|_inf / |u0|_inf = %.3e (%d iterations)" % (err, c.last_info["iterations"])
    # two fixed variables come back exactly; the rest solves the constrained system
    fixed, vals = np.array([1, dim * n - 2]), np.array([0.25, -1.5])
    c.fix_variables(fixed, vals)
    u2 = c.solve(f, rtol=1e-12, maxit=5000)
    assert c.last_info["converged"] == 1
    assert np.array_equal(u2[fixed], vals)
    # the coarse-space preconditioners are refused with a note (as for the scalar operators): the solve runs Jacobi
    c.clear_fixed()
    c.set_preconditioner(M.PRECOND_TWO_LEVEL)
    u3 = c.solve(f, rtol=1e-12, maxit=5000)
    assert "elasticity only" in c.precond_info()["note"]
    assert np.abs(u3 - u0).max() <= 1e-9 * np.abs(u0).max()


@pytest.mark.parametrize("dim,deg", CASES)
def test_lumped_mass(dim, deg):
    import meshfem_amd as M
    m = _mesh(dim, deg, seed=3)
    ref = O.mass_triplets(m, lumped=True).v
    for storage in (0, 1):
        for op, rep in ((M.OP_MASS, 1), (M.OP_MASS_VECTOR, dim)):
            c = _ctx(m, deg, op)
            c.set_option("matrix_storage", storage)
            d = c.mass_lumped()
            assert c.matrix_storage()[0] == bool(storage)
            assert d.shape == (rep * m.num_nodes,)
            assert np.abs(d - np.repeat(ref, rep)).max() < 1e-14 * np.abs(ref).max(), (storage, op)
            c.close()


@pytest.mark.parametrize("dim,deg", CASES)
def test_forced_p1(dim, deg):
    import meshfem_amd as M
    m = _mesh(dim, deg, seed=3)
    m1 = O.FEMMesh(m.elems, m.verts, 1)
    nv = len(m.verts)
    c = _ctx(m, deg, M.OP_LAPLACIAN)
    c.set_operator_degree(1)
    rng = np.random.default_rng(11)
    lumped_ref = O.mass_triplets(m1, lumped=True).v
    for op, trip, N in ((M.OP_LAPLACIAN, O.laplacian_triplets(m1), 1), (M.OP_MASS, O.mass_triplets(m1), 1),
                        (M.OP_MASS_VECTOR, O.mass_triplets(m1), dim)):
        c.set_operator(op)
        s = trip.sum_repeated()
        ri, rj, rv = _expand(s, N)
        A_ref = _full(N * nv, ri, rj, rv)
        for mode in (M.ASSEMBLE_GATHER, M.ASSEMBLE_ATOMIC):
            c.assemble(mode)
            assert c.matrix_info()[0] == nv
            i, j, v = c.export_upper_triplets()
            assert np.array_equal(i.astype(np.int64), ri) and np.array_equal(j.astype(np.int64), rj)      # degree 1: no vanishing integrals
            assert np.abs(v - rv).max() < 1e-13 * np.abs(rv).max()
            x = rng.standard_normal(N * nv)
            ref = A_ref @ x
            assert np.abs(c.apply_K(x) - ref).max() < 1e-12 * np.abs(ref).max()
            if op != M.OP_LAPLACIAN:
                assert np.abs(c.mass_lumped() - np.repeat(lumped_ref, N)).max() < 1e-14 * np.abs(lumped_ref).max()
    if deg == 2:
        with pytest.raises(M.MeshFEMHipError):
            c.set_operator(M.OP_ELASTICITY)
        # a solve on the view: nv unknowns
        c.set_operator(M.OP_MASS)
        u0 = rng.standard_normal(nv)
        u = c.solve(c.apply_K(u0), rtol=1e-12, maxit=5000)
        assert u.shape == (nv,) and np.abs(u - u0).max() <= 1e-9 * np.abs(u0).max()
    # back to the full degree: the elasticity K of the same context is the oracle's (nothing was rebuilt)
    c.set_operator_degree(0)
    c.set_operator(M.OP_ELASTICITY)
    c.material_isotropic(200.0, 0.3)
    c.assemble()
    assert c.matrix_info()[0] == m.num_nodes
    sim = O.Simulator(m.elems, m.verts, deg)
    sim.set_material_constant(O.ElasticityTensor.isotropic(dim, 200.0, 0.3))
    K_ref = sim.assembleStiffnessMatrix().sum_repeated().to_scipy_full_from_upper().toarray()
    K = c.export_scipy().toarray()
    assert np.abs(K - K_ref).max() < 1e-13 * np.abs(K_ref).max()


@pytest.mark.parametrize("dim,deg", CASES)
def test_divergence_and_gradient(dim, deg):
    import meshfem_amd as M
    from meshfem_amd import scalar_operators as S
    m = _mesh(dim, deg, seed=3)
    c = _ctx(m, deg, M.OP_LAPLACIAN)
    rng = np.random.default_rng(13)
    v = rng.standard_normal((len(m.elems), dim))
    if deg == 2:
        with pytest.raises(M.MeshFEMHipError) as ei:
            S.divergence(c, v)
        assert ei.value.code == M._lib.ERR_UNSUPPORTED
        return
    ref = _divergence_numpy(m, v)
    assert np.abs(S.divergence(c, v) - ref).max() < 1e-12 * np.abs(ref).max()
    s = rng.standard_normal(m.num_nodes)
    g_ref = O.grad_u_average(m, s)
    assert np.abs(S.gradient(c, s) - g_ref).max() < 1e-12 * np.abs(g_ref).max()


@pytest.mark.parametrize("dim", [2, 3])
def test_python_mirror(dim):
    """scalar_operators.laplacian / mass_matrix / mass_elasticity with forceP1 and lumped on ONE quadratic context."""
    import meshfem_amd as M
    from meshfem_amd import scalar_operators as S
    m = _mesh(dim, 2, seed=3)
    m1 = O.FEMMesh(m.elems, m.verts, 1)
    c = M.Context(0)
    c.mesh_build(m.elems, m.verts, 2)
    for mesh, p1 in ((m1, True), (m, False), (m1, True)):
        n = mesh.num_nodes
        Lr = O.laplacian_triplets(mesh).sum_repeated().to_scipy_full_from_upper().toarray()
        Mr = O.mass_triplets(mesh).sum_repeated()
        Lg = S.laplacian(None, None, ctx=c, forceP1=p1).toSciPy().toarray()
        assert Lg.shape == (n, n) and np.abs(Lg - Lr).max() < 1e-13 * np.abs(Lr).max()
        Mg = S.mass_matrix(None, None, ctx=c, forceP1=p1).toSciPy().toarray()
        assert np.abs(Mg - Mr.to_scipy_full_from_upper().toarray()).max() < 1e-13 * np.abs(Mr.v).max()
        Mv = S.mass_elasticity(None, None, 2, ctx=c, forceP1=p1)
        ri, rj, rv = _expand(Mr, dim)
        assert Mv.n == dim * n
        _same_triplets(mesh, Mr, dim, Mv.i, Mv.j, Mv.v)
        lump = S.mass_elasticity(None, None, 2, lumped=True, ctx=c, forceP1=p1)
        lr = O.mass_triplets(mesh, lumped=True).v
        assert np.array_equal(lump.i, lump.j) and np.abs(lump.v - np.repeat(lr, dim)).max() < 1e-14 * np.abs(lr).max()


@pytest.mark.timeout(900)
def test_at_size():
    """40^3 grid of quadratic tets (1 536 000 elements) built on the device."""
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(40, 40, 40, [0, 0, 0], [1, 1, 1])
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    vol = c.elem_volumes().sum()
    n = c.n_node
    c.set_operator(M.OP_MASS_VECTOR)
    y = c.apply_K(np.ones(3 * n))
    assert abs(y.sum() - 3 * vol) < 1e-12 * 3 * vol
    x = np.random.default_rng(0).standard_normal((n, 3))
    yv = c.apply_K(x.reshape(-1)).reshape(n, 3)
    c.set_operator(M.OP_MASS)
    ys = np.column_stack([c.apply_K(np.ascontiguousarray(x[:, k])) for k in range(3)])
    assert np.abs(yv - ys).max() < 1e-13 * np.abs(ys).max()
    c.set_operator_degree(1)
    y1 = c.apply_K(np.ones(c.n_vert))
    assert c.matrix_info()[0] == c.n_vert < n
    assert abs(y1.sum() - vol) < 1e-12 * vol
