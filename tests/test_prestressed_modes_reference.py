"""CPU checks of tests/prestress_util.py, the dense truth eigh((K + s Kg)_ff, M_ff) the GPU tests of mfh_modes_prestressed compare against
(docs/design/04_18_prestressed_modes.md), on the four column fixtures of buckling_util under unit axial compression: s = 0 is the unprestressed
spectrum, (sigma, s) and (2 sigma, s / 2) agree, tension stiffens, the first eigenvalue vanishes at the critical factor that the buckling truth
gives and exactly one is negative beyond it, the softening at half the critical load stands where Dunkerley's line puts it, and the first
eigenvalues are separated far beyond the bar of the device comparison. No GPU."""
import numpy as np
import pytest
import scipy.linalg

import buckling_util as B
import prestress_util as P

RTOL_DEVICE = 1e-6           # the rtol of the device solves (tests/test_gpu_prestressed_modes.py)
NEV = 4


@pytest.mark.parametrize("key", P.COLUMNS)
def test_zero_factor_is_the_unprestressed_spectrum(key):
    Kf, _, Mf = P.free_blocks(key)
    lam = P.truth(key, 0.0)[0]
    ref = scipy.linalg.eigh(Kf, Mf, eigvals_only=True)
    err = np.abs(lam - ref).max()
    print("%s: max |lambda(s = 0) - lambda| = %.3e, n eps lambda_max = %.3e" % (key, err, len(ref) * P.EPS * ref[-1]))
    assert np.all(ref > 0) and err <= len(ref) * P.EPS * ref[-1]        # eigh's own accuracy: absolute, on the scale of the largest eigenvalue


def test_doubling_the_stress_and_halving_the_factor_agree():
    key = "strip-P2"
    Kf, Gf, Mf = P.free_blocks(key)
    f = B.free_vars(key)
    G2 = B.Kg_of(key, B.axial_compression(key, 2.0))[f][:, f].toarray()
    s = 0.5 * P.critical_factor(key)
    one = P.dense_spectrum(Kf, Gf, Mf, s)[0]
    two = P.dense_spectrum(Kf, G2, Mf, 0.5 * s)[0]
    assert np.abs(two - one).max() <= len(one) * P.EPS * np.abs(one).max()


@pytest.mark.parametrize("key", P.COLUMNS)
def test_tension_raises_the_first_eigenvalues(key):
    lam0, lamT = P.truth(key, 0.0)[0], P.truth(key, -1.0)[0]
    print("%s: lambda(-cr) / lambda(0) = %s" % (key, lamT[:NEV] / lam0[:NEV]))
    assert np.all(lamT[:NEV] > lam0[:NEV])


@pytest.mark.parametrize("key", P.COLUMNS)
def test_first_eigenvalue_vanishes_at_the_critical_factor(key):
    """the critical factor comes from the buckling truth eigh(Kg_ff, K_ff), the spectrum from eigh((K + s Kg)_ff, M_ff): two factorisations"""
    lam = P.truth(key, 1.0)[0]
    print("%s: critical factor %.6g, |lambda_1| / lambda_2 = %.3e" % (key, P.critical_factor(key), abs(lam[0]) / lam[1]))
    assert lam[1] > 0 and abs(lam[0]) <= 1e-8 * lam[1]


@pytest.mark.parametrize("key", P.COLUMNS)
def test_one_negative_eigenvalue_beyond_the_critical_factor(key):
    lam = P.truth(key, 1.1)[0]
    assert np.count_nonzero(lam < 0) == 1 and lam[0] < 0 < lam[1]
    assert np.all(P.truth(key, 0.9)[0] > 0)


@pytest.mark.parametrize("key", P.COLUMNS)
def test_softening_at_half_the_critical_load(key):
    """lambda_1(0.5 cr) / lambda_1(0): 0.5 if the first vibration and buckling shapes coincided (Dunkerley); they nearly do on a cantilever"""
    r5 = P.truth(key, 0.5)[0][0] / P.truth(key, 0.0)[0][0]
    r9 = P.truth(key, 0.9)[0][0] / P.truth(key, 0.0)[0][0]
    print("%s: lambda_1(s) / lambda_1(0) = %.4f at 0.5, %.4f at 0.9 of the critical factor" % (key, r5, r9))
    assert 0.50 <= r5 <= 0.55
    assert 0.10 <= r9 <= 0.12


@pytest.mark.parametrize("ratio", P.FACTORS)
@pytest.mark.parametrize("key", P.COLUMNS)
def test_first_eigenvalues_are_separated(key, ratio):
    """the device comparison is made value by value: the first NEV + 1 eigenvalues are at least a thousand device bars
    (sqrt(cond2(M_ff)) rtol |lambda|) apart at every load factor the GPU tests solve at"""
    lam, _, defect = P.truth(key, ratio)
    cond = P.cond_of_mass(key)
    gaps = P.relative_gaps(lam, 6)
    bar = np.sqrt(cond) * RTOL_DEVICE
    print("%s at %.1f: %d free, cond2(M_ff) %.3g, lambda %s, smallest relative gap %.4f = %.0f bars, eigh's defect %.2e" %
          (key, ratio, len(lam), cond, lam[:NEV], gaps.min(), gaps.min() / bar, defect))
    assert cond <= 50
    assert gaps.min() >= 0.01 and gaps.min() >= 1000 * bar
