"""CPU checks of tests/buckling_util.py, the restatement the GPU tests of the geometric stiffness and of mfh_buckling compare against
(docs/design/04_16_buckling.md): sigma = I is the oracle's Laplacian, symmetry, translations are in the kernel, the quadratic form of an affine
field, the load factors scale inversely with the prestress, the column fixtures separate their first factors far beyond the bar of the device
comparison, and the first factor of every column stands where Euler's formula puts it (which pins the reference only). No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import buckling_util as B
import modes_util as U

RTOL_DEVICE = 1e-6           # the rtol of the device solves (tests/test_gpu_buckling.py)
NEV = 4
# first load factor against Euler's pi^2 E I / (4 L^2): (factor / Euler - 1) measured with this file's fixtures. Linear elements are stiff in bending
# (+16 / +17 %); the quadratic tets sit within 1 %; the quadratic strip is only three widths long, where the shear deformation Euler's beam leaves
# out lowers the load by 8 %. Asserted with twice the measured deviation as margin.
EULER_DEVIATION = {"col3d-P1": 0.1585, "col3d-P2": -0.0071, "strip-P1": 0.1695, "strip-P2": -0.0846}


def _name(key):
    return key if isinstance(key, str) else "%dD-P%d" % key


def _sigma(key):
    en, pos = B.mesh_tables(key)
    return B.random_symmetric_field(len(en), pos.shape[1])


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_unit_stress_is_the_oracles_laplacian(key):
    from oracle import meshfem_oracle as O
    en, pos = B.mesh_tables(key)
    dim, deg = key
    Ls = sp.csr_matrix(O.laplacian_triplets(U.fem_mesh(key)).sum_repeated().to_scipy_full_from_upper())
    Lv = sp.kron(Ls, sp.identity(dim))
    Kg = B.geometric_stiffness(dim, deg, en, pos, B.uniform_field(len(en), dim, np.eye(dim)))
    err = abs(Kg - Lv).max() / abs(Lv).max()
    print("%s: %.3e of scale" % (_name(key), err))
    assert err <= 1e-13


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_symmetry_and_translations(key):
    en, pos = B.mesh_tables(key)
    dim, deg = key
    Kg = B.geometric_stiffness(dim, deg, en, pos, _sigma(key))
    scale = abs(Kg).max()
    assert abs(Kg - Kg.T).max() <= 1e-14 * scale
    for a in range(dim):
        t = np.zeros((len(pos), dim))
        t[:, a] = 1.0
        assert np.abs(Kg @ t.ravel()).max() <= 1e-13 * scale


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_quadratic_form_of_an_affine_field(key):
    """u = A x has the constant gradient A: u^T Kg u = sum_c grad u_c . sigma grad u_c |Omega| = |Omega| tr(A sigma A^T) for a uniform sigma
    (both element degrees represent an affine field exactly)"""
    import volume_loads_util as VL
    en, pos = B.mesh_tables(key)
    dim, deg = key
    rng = np.random.default_rng(2)
    A = rng.standard_normal((dim, dim))
    S = rng.standard_normal((dim, dim))
    S = S + S.T
    Kg = B.geometric_stiffness(dim, deg, en, pos, B.uniform_field(len(en), dim, S))
    u = (pos @ A.T).ravel()
    vol = VL.geometry(pos, en[:, :dim + 1])[0].sum()
    want = vol * np.trace(A @ S @ A.T)
    got = u @ (Kg @ u)
    print("%s: %.15g against %.15g" % (_name(key), got, want))
    assert abs(got - want) <= 1e-12 * vol * np.abs(A).sum() ** 2 * np.abs(S).max()


def test_doubling_the_stress_halves_the_factors():
    key = "strip-P2"
    one = B.factors_of(B.column_truth(key)[0][:NEV])
    two = B.factors_of(B.dense_truth(key, B.axial_compression(key, 2.0))[0][:NEV])
    assert np.all(np.isfinite(one)) and np.all(np.abs(2.0 * two / one - 1) <= 1e-10)


def test_tension_has_no_finite_factor():
    key = "strip-P1"
    mu = B.dense_truth(key, B.axial_compression(key, -1.0))[0]
    assert mu[0] > 0 and np.all(np.isinf(B.factors_of(mu[:NEV])))


@pytest.mark.parametrize("key", B.COLUMNS)
def test_columns_separate_their_factors(key):
    """the device comparison is made value by value: the first NEV + 1 eigenvalues of every fixture are at least ten device bars
    (sqrt(cond2(K_ff)) rtol |mu|) apart -- no fixture has to be compared as a cluster"""
    mu, _, cond, defect = B.column_truth(key)
    bar = np.sqrt(cond) * RTOL_DEVICE * np.abs(mu[:NEV])
    gaps = np.diff(mu[:NEV + 1])
    print("%s: %d free, cond2 %.3e, factors %s, gaps / bar %s, eigh's defect %.2e" % (key, len(mu), cond, B.factors_of(mu[:NEV]), gaps / bar, defect))
    assert np.all(mu[:NEV] < 0) and np.all(gaps >= 10 * bar)


@pytest.mark.parametrize("key", B.COLUMNS)
def test_first_factor_against_euler(key):
    fac = B.factors_of(B.column_truth(key)[0][:1])[0]
    dev = fac / B.euler_factor(key) - 1
    print("%s: first factor %.6g, Euler %.6g, deviation %+.4f" % (key, fac, B.euler_factor(key), dev))
    assert abs(dev) <= 2 * abs(EULER_DEVIATION[key])
