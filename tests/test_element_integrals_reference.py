"""The batched references of tests/element_integrals_util.py against the oracle's literal (loop by loop) functions, on the small
meshes of tests/test_shape_derivatives.py: all of (2,1), (2,2), (3,1), (3,2), a constant and a per-element general tensor, with and
without the periodic DoF map. Bound: 1e-13 of the largest entry -- the same arithmetic in another order, the bound the suite uses for
the oracle's own literal / batched pairs (test_oracle_delta_ke_literal_vs_batch_vs_finite_differences)."""
import numpy as np
import pytest

import element_integrals_util as U
from oracle import meshfem_oracle as O
from test_shape_derivatives import _grid

RTOL = 1e-13
CASES = [(2, 1), (2, 2), (3, 1), (3, 2)]


def _close(got, ref, what, scale=None):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max() if scale is None else scale
    assert scale > 0 and err <= RTOL * scale, "%s: err %.3e, scale %.3e" % (what, err, scale)


def _sim(dim, deg, field, periodic, seed=0):
    rng = np.random.default_rng(17 * dim + deg + seed)
    V, T = _grid(dim)
    V = U.perturbed(V, 0.06 / (2 if dim == 3 else 3), seed)               # elements of different shapes; periodic faces still match
    sim = O.Simulator(T, V, deg)
    fl = O.flat_len(dim)
    if field:
        sim.set_material_field([O.ElasticityTensor(dim, U.spd(rng, fl)) for _ in range(len(T))])
    else:
        sim.set_material_constant(O.ElasticityTensor(dim, U.spd(rng, fl)))
    if periodic:
        sim.applyPeriodicConditions()
    return sim, V, rng


def _general_strain(dim, rng):
    A = rng.normal(size=(dim, dim))
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("field", [False, True])
@pytest.mark.parametrize("dim,deg", CASES)
def test_batched_references_equal_the_literal_oracle(dim, deg, field, periodic):
    sim, V, rng = _sim(dim, deg, field, periodic)
    s = U.ElemSet.from_sim(sim)
    assert s.n_dof == sim.numDoFs() and (periodic == (s.n_dof < sim.mesh.num_nodes))
    nn = sim.mesh.num_nodes
    u, du = rng.normal(size=(nn, dim)), rng.normal(size=(nn, dim))
    dp = rng.normal(size=V.shape) * 0.05                                   # moves the boundary too
    cs = _general_strain(dim, rng)
    csf = O.flatten_sym(dim, cs)
    # flattening helpers
    _close(U.flatten(dim, cs), csf, "flatten")
    _close(U.unflatten(dim, csf), cs, "unflatten")
    _close(s.C4[0], sim.elem_D(0).rank4(), "rank4")
    # loads. On a periodic mesh with one tensor the constant-strain load is zero up to rounding (every DoF sums a closed star), so the
    # bound is relative to the largest entry of the same load without the DoF map: the size of the terms that cancel.
    free = U.ElemSet(dim, deg, sim.mesh.elem_nodes, V, s.D)
    _close(U.constant_strain_load(s, cs), sim.constantStrainLoad(cs), "constantStrainLoad", np.abs(U.constant_strain_load(free, cs)).max())
    _close(U.constant_strain_load(s, cs, dp), O.delta_constant_strain_load(sim, cs, dp), "deltaConstantStrainLoad",
           np.abs(U.constant_strain_load(free, cs, dp)).max())
    _close(U.apply_delta_K(s, u, dp), O.apply_delta_stiffness_matrix(sim, u, dp), "applyDeltaStiffnessMatrix")
    # per-element fields
    eps = sim.averageStrainField(u)
    _close(U.average_strain(s, u), eps, "averageStrainField")
    _close(s.stress(U.average_strain(s, u)), sim.averageStressField(u), "averageStressField")
    _close(U.delta_average_strain(s, u, du, dp), O.delta_average_strain_field(sim, u, du, dp), "deltaAverageStrainField")
    _close(U.average_gradient(s, u[:, 0]), O.grad_u_average(sim.mesh, u[:, 0]), "gradUAverage")
    for stress in (False, True):
        _close(U.strain_field(s, u, stress), sim.strainField(u, stress=stress), "strainField stress=%d" % stress)
        _close(U.boundary_strain_field(s, u, sim.mesh.bdry_parent, sim.mesh.bdry_elem_verts, stress),
               O.boundary_strain_field(sim, u, stress=stress), "boundary_strain_field stress=%d" % stress)
    # the element loop of homogenizedElasticityTensor
    ref = np.zeros(O.flat_len(dim))
    for e in range(len(eps)):
        ref += sim.vol[e] * sim.elem_D(e).double_contract_flat(eps[e] + csf)
    got, scale = U.longdouble_sum(U.integrated_stress_terms(s, u, csf))
    assert np.abs(got - ref).max() <= RTOL * scale.max()


@pytest.mark.parametrize("field", [False, True])
@pytest.mark.parametrize("dim,deg", CASES)
def test_batched_mutual_energies_and_one_form_equal_the_oracle(dim, deg, field):
    """The mutual energies and their directional derivative against the oracle's (batched) function, the one-form against the literal
    homogenizedElasticityTensorDiscreteDifferential entry by entry (neither depends on the DoF map: per-node fields in, sums and a
    per-vertex field out). The literal one-form takes half a minute on the 192 P2 tets."""
    sim, V, rng = _sim(dim, deg, field, False, seed=1)
    fl = O.flat_len(dim)
    w = [rng.normal(size=(sim.mesh.num_nodes, dim)) * 0.1 for _ in range(fl)]
    dp = rng.normal(size=V.shape) * 0.05
    s = U.ElemSet.from_sim(sim)
    for d in (None, dp):
        got, scale = U.longdouble_sum(U.mutual_energy_terms(s, w, d))
        ref = O.mutual_energies(sim, w, d)
        assert got.shape == ref.shape and np.abs(got - ref).max() <= RTOL * scale.max()
    one = U.mutual_energy_differential(s, w, len(V))
    d = np.einsum("ijvc,vc->ij", one, dp)
    assert np.abs(d - O.mutual_energies(sim, w, dp)).max() <= 1e-12 * np.abs(one).max() * np.abs(dp).sum()   # a sum over every vertex
    lit = O.homogenized_elasticity_tensor_discrete_differential(sim, w, base_cell_volume=1.0)      # [nVert, N, fl, fl]
    _close(np.transpose(one, (2, 3, 0, 1)), lit, "discrete differential")
