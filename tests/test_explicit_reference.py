"""Self-checks of the explicit-dynamics reference (tests/explicit_util.py) on the CPU: the numpy restatements the device tests compare against must
themselves be right. HRZ lumping is positive with the exact total mass where row-sum lumping fails; the two bounds bracket the dense lambda_max;
the recurrence reproduces the closed form of central differences and conserves its invariant."""
import numpy as np
import pytest

from oracle import meshfem_oracle as O

import explicit_util as X
import modes_util as U

KEYS = list(U.SMALL) + [U.BAR]
EPS = U.EPS


@pytest.mark.parametrize("key", KEYS, ids=X.name)
def test_hrz_weights_and_masses(key):
    m = U.fem_mesh(key)
    w = X.hrz_weights(key)
    d = m.K
    assert abs(w.sum() - 1.0) <= 4 * EPS
    if m.deg == 1:
        assert np.allclose(w, 1.0 / (d + 1), rtol=8 * EPS)
    elif d == 2:
        assert np.allclose(w[:3], 3.0 / 57.0, rtol=64 * EPS) and np.allclose(w[3:], 16.0 / 57.0, rtol=64 * EPS)
    else:
        assert np.allclose(w[:4], 1.0 / 36.0, rtol=64 * EPS) and np.allclose(w[4:], 4.0 / 27.0, rtol=64 * EPS)     # 0.02778, 0.14815
    mass, count = X.lumped_mass(key)
    assert np.allclose(np.array([float(q) for q in X.exact_weights(key)]), w, rtol=64 * EPS)
    assert np.all(mass > 0)
    assert abs(mass.sum() - m.N * X.volumes(key).sum()) <= 8 * EPS * len(mass) ** 0.5 * mass.sum()
    rho = X.element_density(key, 5)
    mrho, _ = X.lumped_mass(key, rho)
    assert np.all(mrho > 0) and abs(mrho.sum() - m.N * (rho * X.volumes(key)).sum()) <= 8 * EPS * len(mass) ** 0.5 * mrho.sum()
    if key == (3, 2):
        # the reason explicit stepping was left out: the row sums of the consistent matrix are negative at the vertices of quadratic tets
        rowsum = O.mass_triplets(m, lumped=True).to_scipy().diagonal()
        assert rowsum.min() < 0


@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "free"])
@pytest.mark.parametrize("key", KEYS, ids=X.name)
def test_bounds_bracket_lambda_max(key, clamped):
    K = U.pencil(key)[0]
    fixed = X.fixed_of(key, clamped)
    lam_max = X.lambda_max(key, clamped)
    upper = X.lambda_upper(key, fixed, X.DENSITY)
    est = float(X.power_iteration(K, X.masses(key), fixed, X.default_start(K.shape[0]), 60))
    est_ld = float(X.power_iteration(K, X.masses(key), fixed, X.default_start(K.shape[0]), 60, X.LD))
    print("%s %s: lambdaUpper / lambda_max %.3f, lambdaEst / lambda_max %.5f, float64-longdouble defect of lambdaEst %.2e" %
          (X.name(key), "clamped" if clamped else "free", upper / lam_max, est / lam_max, abs(est - est_ld) / est_ld))
    assert upper >= lam_max >= est * (1 - 64 * EPS)
    assert est >= 0.98 * lam_max
    assert upper <= 5.0 * lam_max


@pytest.mark.parametrize("j", [0, 3])
@pytest.mark.parametrize("key", KEYS, ids=X.name)
def test_dispersion_and_invariant(key, j):
    """Started from mode j of (K, M_L) at rest: u_n = phi cos(n theta), sin(theta / 2) = omega dt / 2; the leapfrog invariant is constant."""
    K = U.pencil(key)[0]
    lam, Phi = X.spectrum(key)
    phi, om = Phi[:, j], np.sqrt(lam[j])
    dt, n_steps = 0.9 * X.dt_crit(key), 200
    Us, _, _, E = X.explicit_direct(K, X.masses(key), X.fixed_of(key), dt, n_steps, phi, np.zeros_like(phi))
    closed = X.dispersion_closed_form(phi, om, dt, n_steps)
    err = np.linalg.norm(Us - closed, axis=1).max() / np.linalg.norm(phi)
    drift = np.abs(E[:, 3] / E[0, 3] - 1).max()
    print("%s mode %d: dispersion error %.2e, invariant drift %.2e" % (X.name(key), j, err, drift))
    assert err <= 1e-9
    assert drift <= 1e-11


@pytest.mark.parametrize("key", KEYS, ids=X.name)
def test_stability_limit(key):
    """0.95 dt_crit: the invariant holds over 2 000 steps from a random state; 1.02 dt_crit blows up."""
    K = U.pencil(key)[0]
    i = X.case_inputs(key, "undamped")
    args = (K, X.masses(key), X.fixed_of(key))
    E = X.explicit_direct(*args, 0.95 * X.dt_crit(key), 2000, i["u0"], i["v0"])[3]
    assert np.abs(E[:, 3] / E[0, 3] - 1).max() <= 1e-11
    with np.errstate(all="ignore"):
        Us = X.explicit_direct(*args, 1.02 * X.dt_crit(key), 2000, i["u0"], i["v0"])[0]
    assert not np.isfinite(Us[-1]).all() or np.abs(Us[-1]).max() > 1e30 * np.abs(Us[0]).max()
    # mass-proportional damping does not lower the limit
    Ud = X.explicit_direct(*args, 0.99 * X.dt_crit(key), 2000, i["u0"], i["v0"], alpha=5.0 * X.omega1(key))[0]
    assert np.abs(Ud[-1]).max() <= np.abs(Ud[0]).max()


@pytest.mark.parametrize("case", ["undamped", "damped"])
@pytest.mark.parametrize("key", KEYS, ids=X.name)
def test_float64_against_longdouble(key, case):
    """The reference's own defect, the unit of the device tests' bars: small, and the chained recurrence equals the uncut one exactly."""
    du, de = X.reference_defect(key, case)
    print("%s %s: float64 against longdouble over 200 steps: snapshots %.2e, energies %.2e" % (X.name(key), case, du, de))
    assert du <= 1e-10 and de <= 1e-11
    K = U.pencil(key)[0]
    i = X.case_inputs(key, case)
    args = (K, X.masses(key), X.fixed_of(key), i["dt"])
    Us, Vs, As, _ = X.reference_run(key, case)
    U2 = X.explicit_direct(*args, 100, Us[100], Vs[100], i["f"], i["amplitude"][100:], i["alpha"], a0=As[100])[0]
    assert np.array_equal(U2, Us[100:])
