"""CPU checks of the modal transient layer (docs/design/04_22_modal_transient.md): the library's coefficient function against mpmath, and the
references of tests/modal_transient_util.py against each other. Only the first part calls the library (the host function
mfh_modal_transient_coeffs needs no device).

Figures of the run that set the constants (printed by every run):
* coefficients: worst error 5.2e-6 of the bar 8 eps S (the library's doubles are the correctly rounded ones almost everywhere); the naive float64
  closed forms miss the bar by 1.5e6 at (1e-6, 0.1) and by 2.5e10 at (1e-2, 1e-5);
* twin on the full basis against the dense exact solution, worst over 3 loads x 3 damping cases: 1.25e-13 (TWIN_DENSE_WORST = 1.3e-13);
* float64 against long-double twin on those cases (every mode on its own scale): 6.0e-14 at most."""
import math

import numpy as np
import pytest

import meshfem_amd as M

import dynamics_util as D
import harmonic_util as H
import modal_transient_util as T
import modal_util as MU
import modes_util as U

EPS = T.EPS
LAMBDAS = (0.0, 1e-6, 1e-2, 1.0, 25.0, 1e4, 1e8)
DTS = (1e-5, 1e-3, 0.1, 10.0)


def _dampings(lam):
    w = math.sqrt(lam)
    return (0.0, 1.0) if lam == 0.0 else (0.0, 0.05 * 2 * w, 2 * w * (1 - 1e-9), 2 * w, 5 * 2 * w)


def _naive(lam, c, dt):
    """The textbook closed forms in float64 (under-damped branch only)."""
    w = math.sqrt(lam)
    xi = c / (2 * w)
    wd = w * math.sqrt(1 - xi * xi)
    e, s, co = math.exp(-xi * w * dt), math.sin(wd * dt), math.cos(wd * dt)
    A11 = e * (co + xi * w / wd * s)
    A12 = e * s / wd
    A21 = -lam * A12
    A22 = e * (co - xi * w / wd * s)
    b0q = (1 - A11) / lam
    b1q = (dt - c * b0q - A12) / lam
    return np.array([A11, A12, b0q, b1q, A21, A22, A12, b0q])


def test_coefficients_against_mpmath():
    """mfh_modal_transient_coeffs within 8 eps S componentwise of mpmath (50 digits, rounded to double) over the grid lambda x dt x c of the design note:
    rigid, under-damped, nearly critical, critical and over-damped modes, omega dt from 1e-8 to 1e5."""
    worst = 0.0
    for lam in LAMBDAS:
        for dt in DTS:
            for c in _dampings(lam):
                got = M.modal_transient_coeffs(lam, c, dt)
                ref = T.mp_coeffs(lam, c, dt)
                assert np.all(np.isfinite(got)), (lam, dt, c, got)
                ratio = np.abs(got - ref) / (8 * EPS * T.natural_scale(lam, c, dt))
                worst = max(worst, ratio.max())
                assert np.all(ratio <= 1.0), (lam, dt, c, got, ref, ratio)
    print("coefficients: worst error %.3e of the bar 8 eps S" % worst)


@pytest.mark.parametrize("lam,dt", [(1e-6, 0.1), (1e-2, 1e-5)])
def test_the_bar_bites_the_naive_closed_forms(lam, dt):
    """The bar is not loose: the textbook float64 closed forms miss it where omega dt is small."""
    ref = T.mp_coeffs(lam, 0.0, dt)
    ratio = np.abs(_naive(lam, 0.0, dt) - ref) / (8 * EPS * T.natural_scale(lam, 0.0, dt))
    print("naive closed forms at (%g, %g): %.3e of the bar" % (lam, dt, ratio.max()))
    assert ratio.max() > 1.0
    got = M.modal_transient_coeffs(lam, 0.0, dt)
    assert np.all(np.abs(got - ref) <= 8 * EPS * T.natural_scale(lam, 0.0, dt))


def test_coefficients_refusals():
    for args in ((-1.0, 0.0, 0.1), (1.0, -0.1, 0.1), (1.0, 0.0, 0.0), (1.0, 0.0, -1.0), (float("nan"), 0.0, 0.1), (1.0, float("inf"), 0.1), (1.0, 0.0, float("inf"))):
        with pytest.raises(M.MeshFEMHipError):
            M.modal_transient_coeffs(*args)
    assert M.modal_transient_coeffs([0.0, 1.0, 4.0], 0.1, 0.01).shape == (3, 8)


def _full_basis_case(load, case, n_steps=200):
    Kf, Mf, free, lam, X = T.fixture56()
    dt, amp = T.loads(T.KEY56, n_steps)[load]
    aR, bR, zeta = T.damping_case(T.KEY56, case)
    f = H.load(T.KEY56, "real")
    coef = T.mp_table(lam, T.mode_damping(lam, aR, bR, zeta), dt)
    return dict(dt=dt, amp=amp, aR=aR, bR=bR, zeta=zeta, f=f, coef=coef, lam=lam, X=X, g=X @ f)


def test_twin_is_the_dense_exact_solution():
    """With the full basis of the 56-unknown fixture the recurrence (mpmath coefficients) reproduces scipy's expm of the first-order system for a
    step, a ramp and a sampled sine, undamped, Rayleigh and per-mode zeta; the float64 twin's own defect against long double per case."""
    worst = 0.0
    for load in ("step", "ramp", "sine"):
        for case in T.DAMPING_CASES:
            p = _full_basis_case(load, case)
            Q, _ = T.twin(p["coef"], p["g"], p["amp"], p["dt"])
            Ue = T.dense_exact(p["f"], p["amp"], p["dt"], p["aR"], p["bR"], p["zeta"])
            dist = np.linalg.norm(T.modal_fields(p["X"], Q) - Ue, axis=1).max() / np.linalg.norm(Ue, axis=1).max()
            defect = T.twin_defect(p["coef"], p["g"], p["amp"], p["dt"])[0]
            print("%s / %s: twin against dense exact %.3e, float64 against long double %.3e" % (load, case, dist, defect))
            worst = max(worst, dist)
            assert defect < 1e-12
    print("worst distance %.3e (TWIN_DENSE_WORST = %.1e)" % (worst, T.TWIN_DENSE_WORST))
    assert worst <= T.TWIN_DENSE_WORST


@pytest.mark.parametrize("case", ["undamped", "rayleigh"])
def test_newmark_moves_towards_the_twin(case):
    """newmark_direct at dt and dt / 2 on the ramp (a load that is piecewise linear at either step): its error against the exact twin at least halves
    -- the least a second-order scheme must do."""
    Kf, Mf, free, lam, X = T.fixture56()
    K, Mm = U.pencil(T.KEY56)
    aR, bR, _ = T.damping_case(T.KEY56, case)
    f = H.load(T.KEY56, "real")
    g = X @ f
    w1 = math.sqrt(lam[0])
    t_end = 2.0 * 2.0 * math.pi / w1
    errs = []
    for n_steps in (80, 160):
        dt = t_end / n_steps
        amp = np.arange(n_steps + 1) / n_steps
        Q, _ = T.twin(T.mp_table(lam, T.mode_damping(lam, aR, bR), dt), g, amp, dt)
        Ut = T.modal_fields(X, Q)
        zero = np.zeros(K.shape[0])
        Un = D.newmark_direct(K, Mm, free, dt, n_steps, zero, zero, f, amp, density=T.DENSITY, damping=(aR, bR))[0]
        errs.append(np.linalg.norm(Un - Ut, axis=1).max() / np.linalg.norm(Ut, axis=1).max())
    print("%s: Newmark against the twin %.3e at dt, %.3e at dt / 2" % (case, errs[0], errs[1]))
    assert errs[1] < errs[0] / 2
