"""The operator of the PCG as a linear map: every instantiated flavour of y = K x -- cluster matrix-free (k_mf_cluster / k_mf_rows and
their batched k_*_nr forms, interleaved right-hand sides in sub-batches), assembled block-CSR (k_spmv, k_spmv_nr, k_spmv_sym), scalar
1x1 operators -- against the plain-C oracle's K mirrored to both triangles and multiplied in FP64, through the test hook
mfh_debug_apply_operator (the path of the batched PCG, apply_op_nr). The p . Ap the kernels fuse into the product (plain dotOut, the
classic and the Chronopoulos-Gear bookkeeping) is compared with x . y_ref, and closed gates must leave y untouched.

Meshes are perturbed grids large enough for several element blocks with interface rows (asserted through mfh_matrix_free_info), so that
the LDS sub-batch offsets, the interface buffer and the second pass all carry data. Bounds: max |y - y_ref| <= 1e-12 max |y_ref|,
|dot - x . y_ref| <= 1e-12 |x| |y_ref| (FP64 sums of ~30 terms per entry in another order)."""
import numpy as np
import pytest
import scipy.sparse as sp

import meshfem_amd as M
from meshfem_amd import _lib as L
from meshfem_amd import grid
from element_integrals_util import MODES, material as _material, perturbed   # one copy, shared with test_gpu_element_integrals.py
from oracle import c_oracle as CO
from oracle import meshfem_oracle as O

pytestmark = pytest.mark.gpu

Y_RTOL = 1e-12
DOT_RTOL = 1e-12
BATCHES = {3: (1, 2, 6), 2: (1, 3)}
UNSUPPORTED = {3: (3, 4, 5), 2: (2, 6)}


def _mesh(dim, small=False, seed=0):
    """3D: 6 x 5 x 4 cells, 2 880 tets; 2D: 20 x 16 quads, 1 280 triangles. Interior vertices moved by up to 4 % of the spacing (the
    boundary stays put, so that the periodic faces still match)."""
    if dim == 3:
        V, T = grid.grid_tet_mesh(*((2, 2, 1) if small else (6, 5, 4)))
    else:
        V, T = grid.grid_tri_mesh(*((3, 2) if small else (20, 16)))
    return perturbed(V, 0.04, seed), np.asarray(T)


def _context(V, T, deg, set_material, periodic, options=()):
    c = M.Context(0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(T, V, deg)
    set_material(c)
    if periodic:
        c.apply_periodic_conditions()
    return c


def _oracle_K(c, V, deg, D, periodic):
    """The oracle's K (upper triangle, reference loop structure) mirrored to the full symmetric matrix, CSR."""
    dim = c.dim
    dof = c.get_dof_map()[0] if periodic else None
    Ap, Ai, Ax, _ = CO.assemble_csc(dim, deg, c.elem_nodes(), V, D, c.n_dof, dof)
    n = dim * c.n_dof
    U = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
    return (U + U.T - sp.diags(U.diagonal())).tocsr()


def _fix_face(c, V, periodic):
    """Fix the nodes on the face x = min (Dirichlet); returns the boolean mask of the fixed rows."""
    dim = c.dim
    pos = c.node_positions()
    nodes = np.nonzero(pos[:, 0] < V[:, 0].min() + 1e-9)[0]
    dofs = c.get_dof_map()[0][nodes] if periodic else nodes
    dofs = np.unique(dofs)
    var = (dofs[:, None] * dim + np.arange(dim)).ravel()
    c.fix_variables(var, np.zeros(len(var)))
    mask = np.zeros(dim * c.n_dof, bool)
    mask[var] = True
    return mask


def check_operator(c, K, fixed, batches, rng, flavours=(0, 1, 2), label=""):
    """Every batch size and flavour, masked and unmasked, against y_ref = K x; dots against x . y_ref; closed gates leave y."""
    n = K.shape[0]
    for nr in batches:
        for masked in (False, True):
            X = rng.standard_normal((nr, n))
            if masked:
                X[:, fixed] = 0.0         # a PCG direction is zero on the fixed rows (mfh_kernels.hip k_mf_cluster: the interface rows' dot skips the mask)
            Yref = (K @ X.T).T
            if masked:
                Yref[:, fixed] = 0.0
            for fl in flavours:
                if fl == 1 and nr > 1:
                    continue
                Y, dots = c.debug_apply_operator(X, masked=masked, flavour=fl)
                what = "%s nr=%d masked=%d flavour=%d" % (label, nr, masked, fl)
                scale = np.abs(Yref).max()
                err = np.abs(Y - Yref).max()
                assert err <= Y_RTOL * scale, "%s: y err %.3e (scale %.3e)" % (what, err, scale)
                ref = np.einsum("ij,ij->i", X, Yref)
                derr = np.abs(dots - ref)
                bound = DOT_RTOL * np.linalg.norm(X, axis=1) * np.linalg.norm(Yref, axis=1)
                assert np.all(derr <= bound), "%s: dot err %s > %s" % (what, derr, bound)
                # the same gate closed: y and the history stay as they were
                if fl in (1, 2):
                    Y0 = rng.standard_normal((nr, n))
                    Yc, dc = c.debug_apply_operator(X, masked=masked, flavour=fl + 2, Y=Y0)
                    assert np.array_equal(Yc, Y0), what + ": closed gate wrote y"
                    assert np.all(dc == 0.0), what + ": closed gate wrote the history"


def _assert_blocks(c, min_blocks=3):
    info = c.matrix_free_info()
    assert info["active"] and info["mode"] == 4, info
    assert info["blocks"] >= min_blocks and info["interface_partials"] > 0, info
    return info


@pytest.mark.timeout(600)
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dim,deg", [(3, 2), (3, 1), (2, 2), (2, 1)])
def test_operator_matches_oracle_every_flavour(dim, deg, mode, periodic):
    """Cluster matrix-free (GEOV on and off where it applies), deterministic cluster and assembled full-storage SpMV on one mesh and
    material: all batch sizes, masked and unmasked, plain / classic / Chronopoulos-Gear, gates open and closed."""
    V, T = _mesh(dim)
    setter, D = _material(mode, dim, len(T))
    rng = np.random.default_rng(7)
    K = None
    variants = [("cluster", ()), ("deterministic", (("deterministic", 1),)), ("assembled", (("matrix_free", 0), ("matrix_storage", 0)))]
    for name, opts in variants:
        c = _context(V, T, deg, setter, periodic, opts)
        if K is None:
            K = _oracle_K(c, V, deg, D, periodic)
        fixed = _fix_face(c, V, periodic)
        if name == "assembled":
            assert not c.matrix_free_info()["active"]
            check_operator(c, K, fixed, BATCHES[dim], rng, label=name)
        elif name == "deterministic":
            _assert_blocks(c)
            check_operator(c, K, fixed, (1, BATCHES[dim][-1]), rng, label=name)
            # bit for bit: the single-vector kernels, the only ones a deterministic solve runs (solve_many and the batched V-cycle keep
            # deterministic contexts on one right-hand side at a time; the batched kernels add in LDS in arrival order)
            X = rng.standard_normal(K.shape[0])
            a, da = c.debug_apply_operator(X, masked=True, flavour=0)
            b, db = c.debug_apply_operator(X, masked=True, flavour=0)
            assert np.array_equal(a, b) and np.array_equal(da, db), "deterministic 1: two applications differ"
        else:
            _assert_blocks(c)
            geov = (1, 0) if mode in ("iso", "general", "ortho") else (1,)
            for g in geov:
                c.set_option("mf_geometry_from_vertices", g)
                check_operator(c, K, fixed, BATCHES[dim], rng, label="%s geov=%d" % (name, g))
        c.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("field", [False, True])
@pytest.mark.parametrize("dim,deg", [(3, 2), (2, 1)])
def test_cluster_block_shapes_match_oracle(dim, deg, field):
    """The block-shape options of the cluster operator: consecutive-element blocks (mf_reorder 0) of 16 / 74 / 100 / 1000 / 4096
    elements (74: the lane stride 37 is not coprime, identity lanes; 1000: a tail block), lane strides 1 / 37 / 64, XCD runs of
    0 / 2 / 3 blocks over 29 blocks of 100 (full windows of 8 G blocks and the identity-mapped tail of xcd_group_item), whole-cell
    blocks (mf_reorder 1). Blocks of 1 000 or more P2 tets do not fit the LDS budget: the context falls back to the two-pass variant,
    which must give the same K x."""
    V, T = _mesh(dim)
    setter, D = _material("iso_field" if field else "iso", dim, len(T))
    rng = np.random.default_rng(11)
    c = _context(V, T, deg, setter, False)
    K = _oracle_K(c, V, deg, D, False)
    fixed = _fix_face(c, V, False)
    nrs = (1, BATCHES[dim][-1])
    settings = [dict(mf_reorder=1), dict(mf_reorder=1, mf_xcd_group=2), dict(mf_reorder=0)]
    settings += [dict(mf_reorder=0, mf_block_elems=be, mf_lane_stride=ls) for be in (16, 74, 100, 1000, 4096) for ls in (1, 37, 64)]
    settings += [dict(mf_reorder=0, mf_block_elems=100, mf_xcd_group=g) for g in (0, 2, 3)]
    for s in settings:
        opts = dict(mf_reorder=1, mf_block_elems=0, mf_lane_stride=37, mf_xcd_group=32)
        opts.update(s)
        for k, v in opts.items():
            c.set_option(k, v)
        info = c.matrix_free_info()
        if info["mode"] != 4:
            assert dim == 3 and opts["mf_block_elems"] >= 1000, (s, info)
            x = rng.standard_normal(K.shape[0])
            assert np.abs(c.apply_K(x) - K @ x).max() <= Y_RTOL * np.abs(K @ x).max()
            continue
        if opts["mf_block_elems"] == 4096:
            assert info["blocks"] == 1 and info["interface_partials"] == 0, (s, info)
        elif opts["mf_block_elems"] == 1000:
            assert info["blocks"] == 2 and info["interface_partials"] > 0, (s, info)          # 1 280 triangles: a tail block of 280
        else:
            assert info["blocks"] >= 3 and info["interface_partials"] > 0, (s, info)
        if opts["mf_block_elems"] == 100 and dim == 3:
            assert info["blocks"] == 29, info
        check_operator(c, K, fixed, nrs, rng, flavours=(0, 2), label=str(s))
    c.close()


@pytest.mark.parametrize("dim,deg", [(3, 2), (3, 1), (2, 2), (2, 1)])
def test_tiny_meshes_match_oracle(dim, deg):
    """One element, and a mesh smaller than one block (no interface rows: k_mf_rows has no work)."""
    rng = np.random.default_rng(5)
    for one in (True, False):
        V, T = _mesh(dim, small=True)
        if one:
            used = np.unique(T[:1])
            remap = np.full(len(V), -1)
            remap[used] = np.arange(len(used))
            V, T = V[used], remap[T[:1]]
        setter, D = _material("general_field", dim, len(T))
        c = _context(V, T, deg, setter, False, (("mf_reorder", 0),))
        K = _oracle_K(c, V, deg, D, False)
        info = c.matrix_free_info()
        assert info["mode"] == 4 and info["blocks"] == 1 and info["interface_partials"] == 0, info
        fixed = np.zeros(K.shape[0], bool)
        fixed[: dim] = True
        c.fix_variables(np.arange(dim), np.zeros(dim))
        check_operator(c, K, fixed, BATCHES[dim], rng, label="one element" if one else "one block")
        c.close()


@pytest.mark.parametrize("dim,deg", [(3, 2), (2, 1)])
def test_upper_storage_spmv_and_refused_hook(dim, deg):
    """matrix_storage 1 with matrix_free 0: c.apply_K runs k_spmv_sym and matches the oracle; the PCG's operator needs both triangles,
    so the hook is refused for every batch size (require_full_storage)."""
    V, T = _mesh(dim)
    setter, D = _material("general_field", dim, len(T))
    c = _context(V, T, deg, setter, False, (("matrix_free", 0), ("matrix_storage", 1)))
    K = _oracle_K(c, V, deg, D, False)
    x = np.random.default_rng(3).standard_normal(K.shape[0])
    assert np.abs(c.apply_K(x) - K @ x).max() <= Y_RTOL * np.abs(K @ x).max()
    assert c.matrix_storage()[0]
    for nr in BATCHES[dim]:
        with pytest.raises(M.MeshFEMHipError) as ei:
            c.debug_apply_operator(np.zeros((nr, K.shape[0])))
        assert ei.value.code == L.ERR_UNSUPPORTED
    c.close()


@pytest.mark.parametrize("dim,deg", [(3, 2), (2, 1)])
def test_scalar_operators_batched_spmv(dim, deg):
    """Laplacian and mass matrix (1 x 1 blocks) through k_spmv_nr for NR 2, 3, 6 and the single-vector kernel, against the oracle's
    triplets (tests/test_scalar_operators.py)."""
    if dim == 3:
        V, T = O.grid_tet_mesh(4, 3, 3)
    else:
        V, Q = O.gen_grid_2d(8, 6)
        V, T = O.quad_tri_subdiv(V, Q)
        V = V[:, :2]
    V = V + 0.04 * np.random.default_rng(2).standard_normal(V.shape) * 0.5
    m = O.FEMMesh(T, V, deg)
    c = M.Context(0)
    c.mesh_build(m.elems, m.verts, deg)
    rng = np.random.default_rng(9)
    for op, trip in ((M.OP_LAPLACIAN, O.laplacian_triplets(m)), (M.OP_MASS, O.mass_triplets(m))):
        c.set_operator(op)
        A = trip.sum_repeated().to_scipy_full_from_upper().tocsr()
        check_operator(c, A, np.zeros(A.shape[0], bool), (1, 2, 3, 6), rng, flavours=(0, 2), label="op %d" % op)
    c.close()


@pytest.mark.parametrize("dim,deg", [(3, 2), (3, 1), (2, 2), (2, 1)])
def test_unsupported_batch_sizes_are_refused(dim, deg):
    """A batch size without kernels is an error (the launchers throw; before, 3D sizes other than 2 ran the NR = 6 kernel past the end
    of the vectors). The context stays usable: a batched solve of 5 right-hand sides still equals 5 single solves."""
    V, T = _mesh(dim)
    setter, D = _material("iso", dim, len(T))
    for opts in ((), (("matrix_free", 0), ("matrix_storage", 0))):
        c = _context(V, T, deg, setter, False, opts)
        _fix_face(c, V, False)
        n = dim * c.n_dof
        for nr in UNSUPPORTED[dim]:
            with pytest.raises(M.MeshFEMHipError) as ei:
                c.debug_apply_operator(np.ones((nr, n)))
            assert ei.value.code == L.ERR_UNSUPPORTED, nr
        F = np.random.default_rng(4).standard_normal((5, n))
        c.set_option("batch_rhs", 1)
        c.set_option("pcg_variant", 1)
        U, infos = c.solve_batch(F, rtol=1e-12)
        for k in range(5):
            u = c.solve(F[k], rtol=1e-12)
            assert np.abs(U[k] - u).max() <= 1e-8 * np.abs(u).max(), k
        c.close()
