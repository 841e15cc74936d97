"""The method of the modal stress recovery in numpy alone (docs/design/04_24_modal_stress.md; tests/modal_stress_util.py): no device.

  * the factor route (C = F F^T, factor fields u_t = B F[:, t], squares summed over t) against the direct double sum sum_jk C_jk s_j^T A s_k on the
    four small meshes, 2D included. Bar, as tests/test_gpu_modal_random.py sets it for the displacement variances:
        10 x max |float64 twin - long-double twin|  +  truncation x lambda_max(A) x max sum_j |s_j|^2      (lambda_max(A) = 3; components: 1)
  * v2, the half sum of squares, equals stress_measures_util.von_mises(flat)^2 to rounding, 2D and 3D
  * A is positive semi-definite; the variance of a hydrostatic state (its null vector in 3D) is never negative in the twin"""
import numpy as np
import pytest

import element_integrals_util as EU
import harmonic_util as H
import modal_random_util as R
import modal_stress_util as S
from modal_stress_util import bars, factor_route, matrices
import modal_util as MU
import modes_util as U
import stress_measures_util as SM
from oracle import meshfem_oracle as O

EPS = S.EPS


def _elem_set(key):
    V, T, deg, _ = U.mesh_arrays(key)
    m = U.fem_mesh(key)
    return S.elem_set(m.N, deg, m.elem_nodes, V, O.ElasticityTensor.isotropic(m.N, U.E_MOD, U.NU).D)


@pytest.mark.parametrize("key", U.SMALL, ids=lambda k: "%dD-P%d" % k)
def test_factor_route_against_the_double_sum(key):
    s = _elem_set(key)
    lam, X = MU.clamped_basis(key)
    m = min(24, len(lam))
    Xn = X[:m].reshape(m, -1, s.N)
    rng = np.random.default_rng(7)
    for name, Cm in matrices(lam, m, rng).items():
        F, piv, trunc = R.psd_factor_twin(Cm)
        (vld, cld), bar_v, bar_c = bars(s, Xn, F, trunc)
        v64, c64 = factor_route(s, Xn, F, np.float64)
        vd, cd = S.quadratic_stress_direct(s, Xn, Cm, True, np.longdouble)
        ev, ec = float(np.abs((v64 - vd).astype(np.float64)).max()), float(np.abs((c64 - cd).astype(np.float64)).max())
        print("%s %s: rank %d, truncation %.3e; von Mises^2 error %.3e (bar %.3e, largest %.3e), components^2 error %.3e (bar %.3e)" %
              (key, name, F.shape[1], trunc, ev, bar_v, float(vd.max()), ec, bar_c))
        assert ev <= bar_v and ec <= bar_c
        assert np.all(v64 >= 0.0) and np.all(c64 >= 0.0)


def test_gradients_of_the_twin_are_the_element_sets():
    for key in U.SMALL:
        s = _elem_set(key)
        gl = S.corner_gradients(s, np.float64)
        assert np.all(np.abs(gl - s.gl) <= 64 * EPS * np.abs(s.gl).max())
        G = S.gradphi_at_nodes(s, s.gl)
        assert np.array_equal(G, EU.gradphi_at(s.deg, s.K, s.gl, EU.interpolant_nodes(s.deg, s.K)))
        u = np.random.default_rng(1).normal(size=(int(s.en.max()) + 1, s.N))
        for stress in (False, True):
            ref = EU.strain_field(s, u, stress)
            got = S.Twin(s, np.float64).corner_field(u, stress)
            assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("dim", [2, 3])
def test_v2_is_the_squared_von_mises_value(dim):
    rng = np.random.default_rng(dim)
    fl = dim * (dim + 1) // 2
    flat = rng.normal(size=(4000, fl)) * 10.0 ** rng.uniform(-3, 3, size=(4000, 1))
    flat[:50, :dim] = flat[:50, :1]                                 # equal normal entries: the cancelling case of the expanded form
    ref = SM.von_mises(flat) ** 2
    got = S.v2(flat)
    size = S.v2_size(np.abs(flat))
    assert np.all(got >= 0.0) and np.all(np.abs(got - ref) <= 16 * EPS * size)
    ld = S.v2(flat.astype(np.longdouble))
    assert np.all(np.abs((got - ld).astype(np.float64)) <= 6 * EPS * got)          # no cancellation: relative to the value itself
    A = S.vm_form(dim)
    assert np.all(np.abs(np.einsum("nc,cd,nd->n", flat, A, flat) - ref) <= 16 * EPS * size)


@pytest.mark.parametrize("dim", [2, 3])
def test_the_von_mises_form_is_positive_semi_definite(dim):
    w = np.linalg.eigvalsh(S.vm_form(dim))
    assert w.min() >= -4 * EPS and abs(w.max() - 3.0) <= 8 * EPS
    if dim == 3:
        assert abs(w.min()) <= 4 * EPS


def test_hydrostatic_state_has_no_negative_variance():
    """u = x (a uniform dilation): hydrostatic strain and, for the isotropic material, hydrostatic stress. In 3D that is A's null vector: the
    variance of the rank-1 covariance C = a^2 is zero up to the rounding of the gradients, and in the twin (a sum of squares) never below zero,
    while the expanded form s^T A s may be."""
    key = (3, 2)
    s = _elem_set(key)
    pos = U.fem_mesh(key).node_pos
    for a in (1.0, 3.7e-5, 2.1e6):
        vm, comp = S.stress_sumsq_twin(s, (a * pos)[None], True, np.float64)
        size, _ = S.stress_sumsq_twin(s, (a * pos)[None], True, np.float64, sizes=True)
        assert np.all(vm >= 0.0) and np.all(vm <= 64 * EPS * size)
        assert np.all(comp[..., :3] > 0.0) and np.all(np.abs(comp[..., 3:]) <= 64 * EPS * comp[..., :3].max())
