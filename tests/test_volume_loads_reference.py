"""The numpy restatement of the volume loads (tests/volume_loads_util.py) on closed forms: the nodal weights of the four element types, the row sums
of the mass coefficients, the divergence theorem for a constant stress (the volume load is the boundary traction load sigma . n of the oracle's
neumannLoad) and the oracle's constantStrainLoad for a strain that is constant over the mesh. No device."""
import numpy as np
import pytest

import element_integrals_util as U
import volume_loads_util as R
from oracle import meshfem_oracle as O

CASES = [(2, 1), (2, 2), (3, 1), (3, 2)]


def _mesh(dim, seed=3):
    if dim == 3:
        V, T = O.grid_tet_mesh(3, 2, 2)
    else:
        V, Q = O.gen_grid_2d(4, 3)
        V, T = O.quad_tri_subdiv(V, Q)
        V = V[:, :2]
    V = V + 0.08 * np.random.default_rng(seed).standard_normal(V.shape)
    return np.ascontiguousarray(V), np.ascontiguousarray(T)


@pytest.mark.parametrize("dim,deg", CASES)
def test_weights(dim, deg):
    w = R.weights(dim, deg)
    nv = dim + 1
    assert abs(w.sum() - 1.0) <= 1e-15
    if deg == 1:
        assert np.allclose(w, 1.0 / nv, rtol=0, atol=1e-16)
    elif dim == 2:
        assert np.allclose(w[:nv], 0.0, rtol=0, atol=1e-16) and np.allclose(w[nv:], 1.0 / 3.0, rtol=0, atol=1e-16)
    else:
        assert np.allclose(w[:nv], -1.0 / 20.0, rtol=0, atol=1e-16) and np.allclose(w[nv:], 1.0 / 5.0, rtol=0, atol=1e-16)
    # the same numbers from a quadrature of sufficient degree (the oracle's rule)
    assert np.abs(w - np.asarray(O.integrated_shape_functions(deg, dim))).max() <= 1e-15


@pytest.mark.parametrize("dim,deg", CASES)
def test_mass_rows_sum_to_the_weights(dim, deg):
    m = R.mass_coefficients(dim, deg)
    assert np.abs(m - m.T).max() == 0.0
    assert np.abs(m.sum(axis=1) - R.weights(dim, deg)).max() <= 1e-16
    assert np.all(np.linalg.eigvalsh(m) > 0)
    # gradient coefficients: the shape functions sum to 1, so their gradients sum to 0 -- every grad l_k gets the same total factor, and the
    # grad l_k sum to 0 themselves; P1 is the identity
    G = R.poly_gradient_coefficients(dim, deg)
    assert np.abs(G.sum(axis=0) - G.sum(axis=0)[0]).max() <= 1e-15
    if deg == 1:
        assert np.array_equal(G, np.eye(dim + 1))


@pytest.mark.parametrize("dim,deg", CASES)
def test_constant_stress_is_the_boundary_traction_load(dim, deg):
    """divergence theorem: int sigma : grad phi_i = int_boundary phi_i sigma n for a constant sigma, on the unit square / cube and on the
    perturbed mesh of the device tests"""
    rng = np.random.default_rng(7 + dim)
    S = rng.standard_normal((dim, dim))
    S = S + S.T
    flat = U.flatten(dim, S)
    for perturb in (False, True):
        if perturb:
            V, T = _mesh(dim)
        else:
            V, T = O.grid_tet_mesh(2, 2, 2) if dim == 3 else (lambda v, q: (O.quad_tri_subdiv(v, q)[0][:, :2], O.quad_tri_subdiv(v, q)[1]))(*O.gen_grid_2d(3, 3))
        sim = O.Simulator(T, V, deg)
        m = sim.mesh
        _, nrm = m.bdry_elem_geometry()
        sim.neumannTraction[:] = nrm @ S.T
        ref = sim.neumannLoad()
        got = R.Mesh(dim, deg, m.elem_nodes, m.node_pos).stress_field_load(np.broadcast_to(flat, (len(T), len(flat))))
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
        interior = np.setdiff1d(np.arange(m.num_nodes), np.asarray(m.bdry_nodes))
        assert len(interior) and np.abs(got[interior]).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("mat", ["iso", "general_field"])
@pytest.mark.parametrize("dim,deg", CASES)
def test_constant_strain_is_the_oracles_constant_strain_load(dim, deg, mat):
    V, T = _mesh(dim)
    sim = O.Simulator(T, V, deg)
    D = U.material(mat, dim, len(T), seed=dim)[1]
    tensors = [O.ElasticityTensor(dim, d) for d in (D if D.ndim == 3 else [D])]
    if D.ndim == 3:
        sim.set_material_field(tensors)
    else:
        sim.set_material_constant(tensors[0])
    E = np.random.default_rng(11).standard_normal((dim, dim))
    E = E + E.T
    ref = sim.constantStrainLoad(E)
    r = R.Mesh(dim, deg, sim.mesh.elem_nodes, sim.mesh.node_pos)
    eps = np.broadcast_to(U.flatten(dim, E), (len(T), dim * (dim + 1) // 2))
    got = r.stress_field_load(r.stress_of_strain(D, eps))
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("dim,deg", CASES)
def test_body_force_totals_and_kinds_agree(dim, deg):
    """sum_i f_i = (sum_e rho_e vol_e) b; a nodal field that is constant, and an element field that is constant, give the constant flavour"""
    V, T = _mesh(dim)
    m = O.FEMMesh(T, V, deg)
    r = R.Mesh(dim, deg, m.elem_nodes, m.node_pos)
    rng = np.random.default_rng(5)
    b, rho = rng.standard_normal(dim), rng.uniform(0.5, 2.0, len(T))
    f = r.body_force_load(b, rho)
    assert np.abs(f.sum(axis=0) - (rho * r.vol).sum() * b).max() <= 1e-14 * np.abs(b).max() * (rho * r.vol).sum()
    scale = np.abs(f).max()
    assert np.abs(r.body_force_load(np.broadcast_to(b, (len(T), dim)).copy(), rho) - f).max() <= 1e-15 * scale
    assert np.abs(r.body_force_load(np.broadcast_to(b, (m.num_nodes, dim)).copy(), rho) - f).max() <= 1e-14 * scale
    # a linear nodal field is interpolated exactly: the first moment against the closed form int x over a simplex = vol x centroid
    A = rng.standard_normal((dim, dim))
    lin = m.node_pos @ A.T
    centroid = np.asarray(V)[np.asarray(T)].mean(axis=1)
    assert np.abs(r.body_force_load(lin).sum(axis=0) - (r.vol[:, None] * (centroid @ A.T)).sum(axis=0)).max() <= 1e-13 * np.abs(lin).max() * r.vol.sum()
