"""Options on the device: a forced-degree-1 view has its context's options whichever of the two was set up first, and an option whose change
makes derived state stale has that state rebuilt by the next use. One representative per kind of state:
  * here, because no other test file sets the option AFTER the state was built: the symbolic phase (chunk_slots), the two-level
    preconditioner (agg_nodes), the choice of MFH_PRECOND_AUTO (auto_stretch_max);
  * elsewhere, on live contexts: the multigrid hierarchy (test_gpu_multigrid.py), the element blocks of the cluster operator and the verdict on
    them (test_gpu_operator_maps.py, test_gpu_parity.py: matrix_free_mode), the sampler grids (test_gpu_field_sampler.py);
  * not tested: the pair lists of the two-pass operator (mf_chunk_rows / mf_chunk_pairs) -- no public call reports their chunking, so a
    rebuild cannot be told from a reuse; the placement trials (placement_trials) -- they skip value buffers below 256 MB, which no test of a
    few seconds allocates (test_gpu_arena.py runs them once, on 331 776 elements)."""
import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import grid

pytestmark = pytest.mark.gpu


def _view_solve(order, value):
    """Laplacian of the vertices of a quadratic mesh, vertex 0 fixed to `value`; order: "option_first" | "view_first" | "no_option" """
    V, T = grid.grid_tet_mesh(3, 3, 3)
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    c.set_operator(M.OP_LAPLACIAN)
    c.set_option("deterministic", 1)
    if order == "option_first":
        c.set_option("solve_homogeneous", 1)
    c.set_operator_degree(1)
    if order == "view_first":
        c.set_option("solve_homogeneous", 1)
    c.fix_variables([0], [value])
    f = np.random.default_rng(3).standard_normal(len(V))
    u = c.solve(f, rtol=1e-12, maxit=5000)
    assert c.last_info["converged"] and c.matrix_info()[0] == len(V)
    c.close()
    return u


def test_view_has_its_contexts_options_in_either_order():
    """solve_homogeneous reaches mfh_solve on the view (solve_one reads it on the context it solves on): set before the view exists it must
    act exactly as set afterwards. Under "deterministic" the two solves are the same arithmetic: equal bits."""
    ua, ub, uc = (_view_solve(o, 2.5) for o in ("option_first", "view_first", "no_option"))
    assert np.array_equal(ua, ub)
    # the inhomogeneous solve adds the harmonic extension of the fixed value, which with natural conditions everywhere else is the constant
    # 2.5 (K 1 = 0); to the solver's accuracy: rtol 1e-12 times the condition number of the pinned 199-vertex Laplacian (~1e3) on |u| <~ 1e2
    assert uc[0] == 2.5
    assert np.abs((uc - ua)[1:] - 2.5).max() < 1e-6 * max(1.0, np.abs(uc).max())


def _cantilever():
    V, T = grid.grid_tet_mesh(3, 3, 3)
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    c.material_isotropic(200.0, 0.35)
    c.bc_dirichlet_box([-1e-4] * 3, [1e-4, 1.0001, 1.0001], [0, 0, 0], relative=True)
    c.bc_neumann_box([0.9999, -1e-4, -1e-4], [1.0001, 1.0001, 1.0001], [0, -10, 0], kind=M.NEUMANN_FORCE, relative=True)
    return c


def test_chunk_slots_after_assembly_rebuilds_the_symbolic_phase():
    c = _cantilever()
    c.assemble()
    s0, K0 = c.symbolic_sizes(), c.export_scipy()
    assert s0["chunk_slots"] == 256
    c.set_option("chunk_slots", 192)
    with pytest.raises(M.MeshFEMHipError) as ei:                          # dropped at once
        c.symbolic_sizes()
    assert ei.value.code == M._lib.ERR_STATE
    c.assemble()
    s1, K1 = c.symbolic_sizes(), c.export_scipy()
    assert s1["chunk_slots"] == 192 and s1["n_chunk"] > s0["n_chunk"] and s1["n_contrib"] == s0["n_contrib"]
    assert abs(K1 - K0).max() <= 1e-13 * abs(K0).max()
    c.close()


def test_agg_nodes_after_a_solve_rebuilds_the_two_level_preconditioner():
    c = _cantilever()
    c.set_preconditioner(M.PRECOND_TWO_LEVEL)
    # bins per axis = round(extent / H), H^3 = volume x agg_nodes / DoFs (build_aggregates): 2 x 2 x 2 bins for 150 on the 3 x 3 x 3 box with
    # its 1 153 nodes, 4 x 4 x 4 for 24
    c.set_option("agg_nodes", 150)
    u0 = c.sim_solve(rtol=1e-10)
    p0 = c.precond_info()
    assert c.last_info["converged"] and p0["note"] == "" and p0["aggregates"] > 1
    c.set_option("agg_nodes", 24)
    u1 = c.sim_solve(rtol=1e-10)
    p1 = c.precond_info()
    assert c.last_info["converged"] and p1["note"] == ""
    assert p1["aggregates"] > p0["aggregates"] and p1["coarse_dim"] == 6 * p1["aggregates"]
    assert np.linalg.norm(u1 - u0) < 1e-7 * np.linalg.norm(u0)
    c.close()


def test_auto_stretch_max_after_a_choice_makes_precond_auto_choose_again():
    """a 4 : 1 : 1 box has stretch 4 (test_gpu_multigrid.py): below the default threshold 8 the V-cycle, above a threshold of 2 the two-level
    preconditioner; the solution is the same to the tolerance that file uses between these two preconditioners at rtol 1e-10"""
    V, T = grid.grid_tet_mesh(3, 3, 3, [0, 0, 0], [4, 1, 1])
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    c.material_isotropic(200.0, 0.35)
    c.bc_dirichlet_box([-1e-9, -99, -99], [1e-9, 99, 99], [0, 0, 0])
    c.bc_neumann_box([4 - 1e-9, -99, -99], [4 + 1e-9, 99, 99], [0, -1, 0], kind=M.NEUMANN_TRACTION)
    c.set_preconditioner(M.PRECOND_AUTO)
    u0 = c.sim_solve(rtol=1e-10, maxit=5000)
    kind, is_auto, stretch = c.precond_choice()
    assert is_auto and kind == M.PRECOND_MULTIGRID and abs(stretch - 4.0) <= 1e-6 * stretch
    c.set_option("auto_stretch_max", 2)
    kind, is_auto, stretch = c.precond_choice()
    assert is_auto and kind == M.PRECOND_TWO_LEVEL and abs(stretch - 4.0) <= 1e-6 * stretch
    u1 = c.sim_solve(rtol=1e-10, maxit=5000)
    assert c.last_info["converged"] and np.linalg.norm(u1 - u0) <= 1e-7 * np.linalg.norm(u0)
    c.set_option("auto_stretch_max", 8)
    assert c.precond_choice()[0] == M.PRECOND_MULTIGRID
    c.close()
