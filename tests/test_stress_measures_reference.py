"""tests/stress_measures_util.py (the numpy restatement of VonMises.hh, SymmetricMatrix.hh eigenvalues and FieldPostProcessing.hh that the
GPU tests compare the device kernels with) on closed forms. No device."""
import numpy as np
import pytest

import stress_measures_util as R


def _uniaxial(dim, axis, s):
    A = np.zeros((dim, dim))
    A[axis, axis] = s
    return R.flatten(A)


@pytest.mark.parametrize("dim", [2, 3])
def test_uniaxial_is_abs_sigma(dim):
    for axis in range(dim):
        for s in (2.5, -7.0):
            assert abs(R.von_mises(_uniaxial(dim, axis, s)) - abs(s)) < 1e-15 * abs(s)


@pytest.mark.parametrize("dim", [2, 3])
def test_pure_shear_is_sqrt3_tau(dim):
    for i in range(dim):
        for j in range(i + 1, dim):
            for tau in (1.75, -0.3):
                A = np.zeros((dim, dim))
                A[i, j] = A[j, i] = tau
                assert abs(R.von_mises(R.flatten(A)) - np.sqrt(3.0) * abs(tau)) < 4e-16 * np.sqrt(3.0) * abs(tau)


def test_hydrostatic_is_zero_3d():
    assert R.von_mises(R.flatten(-4.2 * np.eye(3))) == 0.0


def test_2d_value_is_the_norm_of_the_reference_extractor():
    """vonMisesExtractor<2> (VonMises.hh:88-98): D(0,0) = D(1,1) = a, D(0,1) = b, D(2,2) = 1/2 sqrt(3/2), applied by doubleContract to the
    flattened matrix with its shear entry doubled; frobeniusNormSq counts the shear entry of the result twice."""
    a, b, d22 = -np.sqrt(2.0 - np.sqrt(3.0)) / 2.0, np.sqrt(2.0 + np.sqrt(3.0)) / 2.0, 0.5 * np.sqrt(1.5)
    D = np.array([[a, b, 0.0], [b, a, 0.0], [0.0, 0.0, d22]])
    rng = np.random.default_rng(0)
    s = rng.normal(size=(200, 3))
    v = (s * np.array([1.0, 1.0, 2.0])) @ D.T
    ref = np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2 + 2.0 * v[:, 2] ** 2)
    assert np.abs(R.von_mises(s) - ref).max() < 1e-14 * np.abs(s).max()
    # and that is the von Mises value of the 3D stress with s_zz = s_xz = s_yz = 0
    s3 = np.zeros((200, 6))
    s3[:, 0], s3[:, 1], s3[:, 5] = s[:, 0], s[:, 1], s[:, 2]
    assert np.abs(R.von_mises(s3) - ref).max() < 1e-14 * np.abs(s).max()


@pytest.mark.parametrize("dim", [2, 3])
def test_eigenvalues_are_eigvalsh(dim):
    rng = np.random.default_rng(dim)
    A = rng.normal(size=(300, dim, dim))
    A = A + np.swapaxes(A, 1, 2)
    f = R.flatten(A)
    assert np.array_equal(R.unflatten(f), A)
    assert np.array_equal(R.eigenvalues(f), np.linalg.eigvalsh(A))
    lam, V = R.eigen_decomposition(f)
    assert np.all(np.diff(lam, axis=1) >= 0)
    assert np.abs(A @ V - V * lam[:, None, :]).max() < 1e-13 * np.abs(A).max()


def _two_triangles():
    # vertices 0..3, elements (0 1 2) of area 1/2 and (1 3 2) of area 1: vertices 1 and 2 are shared
    corner_nodes = np.array([[0, 1, 2], [1, 3, 2]])
    vol = np.array([0.5, 1.0])
    return corner_nodes, vol


def test_vertex_average_of_a_constant_is_the_constant():
    cn, vol = _two_triangles()
    c = np.array([1.5, -2.0, 0.25])
    for nq in (1, 3):
        out = R.vertex_averaged(cn, vol, np.broadcast_to(c, (2, nq, 3)), 4)
        assert np.abs(out - c).max() < 1e-15 * np.abs(c).max()


def test_vertex_average_by_hand():
    cn, vol = _two_triangles()
    f = np.array([[1.0, 2.0, 3.0], [10.0, 20.0, 30.0]])[..., None] * np.array([1.0, -1.0])      # [2 elements, 3 corners, 2 components]
    out = R.vertex_averaged(cn, vol, f, 4)
    expect = np.array([1.0,                                     # vertex 0: corner 0 of element 0 alone
                       (0.5 * 2.0 + 1.0 * 10.0) / 1.5,          # vertex 1: corner 1 of element 0, corner 0 of element 1
                       (0.5 * 3.0 + 1.0 * 30.0) / 1.5,          # vertex 2: corner 2 of both
                       20.0])                                   # vertex 3: corner 1 of element 1 alone
    assert np.abs(out[:, 0] - expect).max() < 1e-15 * 30 and np.array_equal(out[:, 1], -out[:, 0])
    # per-element constants: every corner takes the element's value
    g = np.array([[[4.0]], [[7.0]]])
    out = R.vertex_averaged(cn, vol, g, 4)[:, 0]
    assert np.abs(out - np.array([4.0, (0.5 * 4 + 7.0) / 1.5, (0.5 * 4 + 7.0) / 1.5, 7.0])).max() < 1e-15 * 7
