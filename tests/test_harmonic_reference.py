"""CPU tests of the frequency-response reference (tests/harmonic_util.py) against closed forms, of the numpy COCG stand-in of the device loop against
that reference, and of mfh_harmonic's argument checks on a host-only context. Bars of the reference against itself: the modal sum and the static
limit go through one more factorisation or an eigendecomposition of the same matrices, so they get 1e4 eps cond-free headroom = 1e-10 relative
(measured: below 1e-12); the dissipation identity is an algebraic identity of the solved system and gets the same."""
import ctypes as C

import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import _lib

import harmonic_util as H
import modes_util as U

RTOL = 1e-12


def _name(key):
    return key if isinstance(key, str) else "%dD-P%d" % key


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_modal_sum(key):
    """Rayleigh damping is diagonal in the modes: x_j^T M u^ = x_j^T f / (zK lam_j + zM) for the five smallest modes (X M-orthonormal at density 1)."""
    lam, X, _, defect = U.clamped_truth(key)
    _, Mm = U.pencil(key)
    free = H.free_of(key)
    Mf = Mm[free][:, free]
    f = H.load(key)[free]
    ref = H.reference(key, "rayleigh")
    worst = 0.0
    for k, w in enumerate(H.sweep_omegas(key)):
        zK, zM = H.coefficients(key, "rayleigh", float(w))
        q = X[:, :5].T @ (Mf @ ref[k][free])
        closed = (X[:, :5].T @ f) / (zK * lam[:5] + zM)
        worst = max(worst, float(np.abs(q - closed).max() / np.abs(closed).max()))
    print("%s: modal coordinates against the closed form %.3e (scipy's orthonormality defect %.1e)" % (_name(key), worst, defect))
    assert worst <= 1e-10


@pytest.mark.parametrize("case", list(H.CASES))
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_static_limit_and_dissipation(key, case):
    K, Mm = U.pencil(key)
    free = H.free_of(key)
    Kf, Mf = K[free][:, free], H.DENSITY * Mm[free][:, free]
    f = H.load(key)[free]
    ref = H.reference(key, case)
    (aR, bR), eta = H.damping(key, case)
    if case == "undamped":
        static = H._lu(Kf).solve(f)
        err = H.rel_l2(ref[0][free], static)
        print("%s: omega = 0 against the static solve %.3e" % (_name(key), err))
        assert err <= 1e-10
        assert np.all(ref.imag == 0.0)
    for k, w in enumerate(H.sweep_omegas(key)):
        u = ref[k][free]
        lhs = np.vdot(u, f).imag
        uKu, uMu = np.vdot(u, Kf @ u).real, np.vdot(u, Mf @ u).real
        rhs = w * (aR * uMu + bR * uKu) + eta * uKu
        assert abs(lhs - rhs) <= 1e-10 * abs(np.vdot(u, f)), (k, lhs, rhs)


@pytest.mark.parametrize("precond", ["Kinv", "jacobi"])
@pytest.mark.parametrize("case", ["undamped", "rayleigh"])
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_cocg_standin(key, case, precond):
    """The COCG recurrence with a real SPD preconditioner converges at every test frequency, the indefinite undamped ones included, and lands within
    1e2 rtol of the direct solve (worst measured over the 80 runs: see docs/design/04_17_harmonic.md); its true residual within 1e2 rtol."""
    runs = H.standin_runs(key, case, precond, RTOL)
    for k, r in enumerate(runs):
        print("%s %s %s omega[%d]: %d iterations, error %.2e, true residual %.2e, min |pZp| %.1e" %
              (_name(key), case, precond, k, r["iterations"], r["err"], r["true_res"], r["min_pZp"]))
    assert all(r["iterations"] >= 0 for r in runs)
    assert max(r["err"] for r in runs) <= 1e2 * RTOL
    assert max(r["true_res"] for r in runs) <= 1e2 * RTOL
    if precond == "Kinv":
        assert runs[0]["iterations"] == 1           # omega = 0: B Z = (1 + i eta) I


def _raw(c, prm, om, f, pv=None, n_probe=0, pout=None):
    n = c.bs * c.n_dof
    om = _lib.as_f64(np.asarray(om, dtype=np.float64))
    f = _lib.as_f64(np.asarray(f, dtype=np.float64))
    fld = np.zeros((max(len(om), 1), 2, n))
    info = _lib.HarmonicInfo()
    return c.lib.mfh_harmonic(c.h, None if prm is None else C.byref(prm), _lib.ptr(om), _lib.ptr(f), None, _lib.ptr(pv), n_probe, _lib.ptr(pout),
                              _lib.ptr(fld), None, None, C.byref(info))


def test_host_only_context_checks_arguments_first():
    """Every invalid-parameter case of mfh_harmonic is refused with MFH_ERR_INVALID before any device work -- so a host-only context refuses them
    too -- and a valid call on it fails with MFH_ERR_HIP (no CPU fallback)."""
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(1, 1, 1)
    c = M.Context(-1)
    c.mesh_build(T, V, 1)
    n = 3 * c.n_dof
    f = np.ones(n)
    good = dict(density=1.0, damping=(0.0, 0.0), loss_factor=0.0, rtol=1e-8, maxit=100)

    def call(omega=(1.0,), **kw):
        args = dict(good)
        args.update(kw)
        return c.harmonic(np.asarray(omega, dtype=np.float64), f, **args)
    bad = {
        "omega not finite": lambda: call(omega=(1.0, np.nan)),
        "omega infinite": lambda: call(omega=(np.inf,)),
        "omega negative": lambda: call(omega=(-1.0,)),
        "omega = 0 without fixed variables": lambda: call(omega=(0.0,)),
        "density 0": lambda: call(density=0.0),
        "density negative": lambda: call(density=-1.0),
        "rayleigh mass negative": lambda: call(damping=(-0.1, 0.0)),
        "rayleigh stiffness negative": lambda: call(damping=(0.0, -0.1)),
        "loss factor negative": lambda: call(loss_factor=-0.01),
        "rtol 0": lambda: call(rtol=0.0),
        "rtol 1": lambda: call(rtol=1.0),
        "maxit 0": lambda: call(maxit=0),
        "probe out of range": lambda: call(probes=[n]),
        "probe negative": lambda: call(probes=[-1]),
    }
    for name, fn in bad.items():
        with pytest.raises(M.MeshFEMHipError) as ei:
            fn()
        assert ei.value.code == _lib.ERR_INVALID, name
    P = _lib.HarmonicParams
    pv = np.zeros(1, dtype=np.int64)
    raw = {
        "null params": lambda: _raw(c, None, [1.0], f),
        "nFreq negative": lambda: _raw(c, P(1.0, 0.0, 0.0, 0.0, 1e-8, -1, 100, 0), [1.0], f),
        "unknown flag": lambda: _raw(c, P(1.0, 0.0, 0.0, 0.0, 1e-8, 1, 100, 2), [1.0], f),
        "probes without their output": lambda: _raw(c, P(1.0, 0.0, 0.0, 0.0, 1e-8, 1, 100, 0), [1.0], f, pv, 1, None),
    }
    for name, fn in raw.items():
        assert fn() == _lib.ERR_INVALID, name
    with pytest.raises(M.MeshFEMHipError) as ei:
        call(probes=[0, n - 1])
    assert ei.value.code == _lib.ERR_HIP
    c.fix_variables(np.arange(3, dtype=np.int64))
    with pytest.raises(M.MeshFEMHipError) as ei:
        call(omega=(0.0, 1.0))                      # with fixed variables omega = 0 is a valid frequency
    assert ei.value.code == _lib.ERR_HIP
    c.close()
