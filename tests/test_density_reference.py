"""CPU checks of tests/density_util.py, the restatement the GPU tests of the per-element density compare against: it is pinned against three
independent computations -- the oracle's unit-density mass matrix, the body-force restatement of volume_loads_util, the rigid-body mass matrix
from the closed-form mass properties -- and the bimaterial pencil is shown to separate its lowest modes far beyond the tolerance of the device
comparison. No GPU."""
import numpy as np
import pytest

import density_util as DU
import modes_util as U
import volume_loads_util as VL

RTOL_MODES = 1e-6            # the rtol of the device mode solves (tests/test_gpu_density.py, tests/test_gpu_modes.py)


def _name(key):
    return "%dD-P%d" % key


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_unit_density_is_the_oracles_mass_matrix(key):
    M1, Mo = DU.M_rho(key), U.pencil(key)[1]
    err = abs(M1 - Mo).max() / abs(Mo).max()
    print("%s: %.3e of scale" % (_name(key), err))
    assert err <= 1e-13


@pytest.mark.parametrize("name", DU.FIELDS)
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_product_is_the_body_force_load_of_a_nodal_field(key, name):
    """M_rho b = sum_e rho_e int_e phi_i (sum_j phi_j b_j): the MFH_BODY_NODE load of volume_loads_util, written without a matrix"""
    en, pos = DU.mesh_tables(key)
    dim, deg = key
    rho = DU.field(key, name)
    b = np.random.default_rng(3).standard_normal(pos.shape)
    load = VL.Mesh(dim, deg, en, pos).body_force_load(b, rho)
    got = (DU.M_rho(key, name) @ b.ravel()).reshape(load.shape)
    err = np.abs(got - load).max() / np.abs(load).max()
    print("%s %s: %.3e of scale" % (_name(key), name, err))
    assert err <= 1e-13


@pytest.mark.parametrize("name", DU.FIELDS)
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_rigid_body_mass_matrix(key, name):
    """Z^T M_rho Z for the rigid-body modes about the centre of mass: mass I, the inertia about the centre, no coupling. The rigid fields are
    linear in x, so their nodal interpolation is exact on both degrees."""
    en, pos = DU.mesh_tables(key)
    dim = key[0]
    props = DU.mass_properties(dim, en, pos, DU.field(key, name))
    Z = U.rigid_modes(pos)                                           # rotations about the centroid of the nodes
    s = props["com"] - pos.mean(axis=0)
    at_s = U.rigid_modes(np.array([s, -s]))[:dim].copy()             # the rotation fields at the point s (the pair has mean 0)
    at_s[:, :dim] = 0.0
    Zc = Z - np.tile(at_s, (len(pos), 1))                            # ... about the centre of mass
    got = Zc.T @ (DU.M_rho(key, name) @ Zc)
    ref = DU.rigid_mass_matrix(dim, props)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    terr = np.abs(got[:dim, :dim] - ref[:dim, :dim]).max() / props["mass"]
    print("%s %s: %.3e of scale (translation block %.3e)" % (_name(key), name, err, terr))
    assert err <= 1e-12


def test_mass_properties_of_a_known_body():
    """the closed forms on a body whose integrals are known: the unit cube at unit density, mass 1, centre (1/2, 1/2, 1/2), S = I / 12"""
    from oracle import meshfem_oracle as O
    V, T = O.grid_tet_mesh(2, 2, 2, [0, 0, 0], [1, 1, 1])
    p = DU.mass_properties(3, T, V)
    assert abs(p["mass"] - 1.0) <= 1e-14 and np.abs(p["com"] - 0.5).max() <= 1e-14
    assert np.abs(p["second_moment"] - np.eye(3) / 12.0).max() <= 1e-14
    assert np.abs(p["inertia"] - np.eye(3) / 6.0).max() <= 1e-14


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_bimaterial_modes_are_separated(key):
    """The eight smallest clamped eigenvalues of the bimaterial pencil lie at least 100 bars of the device comparison apart (bar = sqrt(cond2(M_ff))
    rtol lambda): a list shifted by one mode cannot pass that comparison."""
    lam, _, cond, _ = DU.clamped_truth(key, "bimaterial")
    gap = (np.diff(lam[:9]) / lam[:8]).min()
    bar = np.sqrt(cond) * RTOL_MODES
    print("%s: smallest relative gap %.3e, bar %.3e" % (_name(key), gap, bar))
    assert gap >= 100 * bar
