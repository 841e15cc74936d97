"""The reference recurrences of tests/pencil_iterates_util.py against themselves and against the direct solves: no device.

The rounding floor of the reference -- the relative gap between its FP64 and its extended-precision walk at every k <= 8, of the iterate and of
the scalars r.z, p.Ap, r.r in their scales -- is printed per input and held to FLOOR_MAX = 1e-11 for every input of
tests/test_gpu_pencil_iterates.py: every small mesh of modes_util, the two Newmark pencils (from zero and from the warm start), every damping
case of harmonic_util at each of its five frequencies, real and complex load. The bound of the device tests, tau_k = max(1e-12, 100 gap_k), is
derived from it; an input that does not meet the floor is to be replaced, not skipped. Measured (iterate / scalars): Newmark pencils 1.1e-15 /
3.1e-15; harmonic inputs <= 1.1e-12 / 4.1e-12 but (2, 1) undamped at mid(omega_8, omega_9) under the complex load with 1.4e-12 / 8.7e-12; from the
warm start <= 1.6e-13 / 4.0e-12.

Run to convergence, the same recurrences land on the splu solutions of harmonic_util / dynamics_util."""
import numpy as np
import pytest

import dynamics_util as D
import harmonic_util as H
import modes_util as U
import pencil_iterates_util as R


def _name(key):
    return "%dD-P%d" % key


def _report(what, ref):
    print("%s: floor of the iterate %.2e, of the scalars %.2e (k <= %d)" % (what, ref.gap_x.max(), ref.gap_s.max(), R.KMAX))
    assert ref.gap_x.max() <= R.FLOOR_MAX and ref.gap_s.max() <= R.FLOOR_MAX, (what, ref.gap_x, ref.gap_s)
    assert np.all(ref.tau_x <= 100 * R.FLOOR_MAX) and np.all(ref.tau_x >= R.TAU_ORACLE)


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_floor_of_the_newmark_pcg(key):
    b, x0 = R.newmark_rhs(key)
    for name, (cK, cM) in R.newmark_pencils(key).items():
        for start in (None, x0):
            ref = R.pcg_reference(key, cK, cM, b, start)
            _report("%s %s %s" % (_name(key), name, "cold" if start is None else "warm"), ref)
            assert len(ref.x) == R.KMAX + 1 and len(ref.pAp) == R.KMAX and len(ref.rz) == R.KMAX + 1
            assert np.all(ref.pAp > 0) and np.all(ref.rz > 0)          # an SPD pencil under an SPD preconditioner


@pytest.mark.parametrize("case", list(H.CASES))
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_floor_of_the_harmonic_cocg(key, case):
    for w in H.sweep_omegas(key):
        zK, zM, cM = R.harmonic_inputs(key, case, w)
        for kind in R.KINDS:
            ref = R.cocg_reference(key, zK, zM, cM, H.load(key, kind))
            _report("%s %s omega %.4f %s" % (_name(key), case, w, kind), ref)
    # from a non-zero start vector (the warm start of a sweep): the solution of the previous frequency
    om = H.sweep_omegas(key)
    zK, zM, cM = R.harmonic_inputs(key, case, om[2])
    ref = R.cocg_reference(key, zK, zM, cM, H.load(key, "complex"), x0=H.reference(key, case, "complex")[1])
    _report("%s %s omega %.4f warm" % (_name(key), case, om[2]), ref)


def test_the_cocg_is_the_recurrence_of_harmonic_util():
    """the same iterate as harmonic_util.cocg at its stop, and a conjugated dot product is another walk (what the device tests must notice)"""
    key, case = (2, 2), "rayleigh"
    Kf, Mf, free, _ = R.free_pencil(key)
    w = H.sweep_omegas(key)[2]
    zK, zM, cM = R.harmonic_inputs(key, case, w)
    f = H.load(key, "complex")[free]
    Dm = R.jacobi_matrix(key, 1.0, cM)
    x, its, _, _ = H.cocg((zK * Kf + zM * Mf).tocsr(), f, lambda r: Dm @ r, 1e-10)
    walk = R.cocg_walk(Kf, Mf, zK, zM, R.jacobi_apply(key, 1.0, cM), f, None, its + 5, rowsum=False, rtol=1e-10, keep=False)
    assert walk.k_stop == its and R.rel(walk.x[-1], x) <= 1e-9
    ref = R.cocg_reference(key, zK, zM, cM, H.load(key, "complex"))
    r0 = f
    z0 = Dm @ r0
    assert abs(ref.rz[0] - r0 @ z0) <= 1e-13 * abs(r0 @ z0)
    assert abs(ref.rz[0] - np.vdot(r0, z0)) > 1e-3 * abs(ref.rz[0])          # r^T z, not r^H z


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_converged_reference_against_the_direct_solves(key):
    """rtol 1e-12; the bar of the device tests against the same direct solves, 1e3 rtol (tests/test_gpu_harmonic.py, tests/test_gpu_dynamics.py)"""
    Kf, Mf, free, _ = R.free_pencil(key)
    rtol, bar = 1e-12, 1e-9
    worst = 0.0
    for case in H.CASES:
        direct = H.reference(key, case, "complex")
        for q, w in enumerate(H.sweep_omegas(key)):
            zK, zM, cM = R.harmonic_inputs(key, case, w)
            walk = R.cocg_walk(Kf, Mf, zK, zM, R.jacobi_apply(key, 1.0, cM), H.load(key, "complex")[free], None, 20000, rowsum=False, rtol=rtol, keep=False)
            assert walk.k_stop is not None
            worst = max(worst, R.rel(walk.x[-1], direct[q][free]))
    print("%s: converged COCG against splu %.2e" % (_name(key), worst))
    assert worst <= bar
    b, _ = R.newmark_rhs(key)
    for name, (cK, cM) in R.newmark_pencils(key).items():
        A = (cK * Kf + cM * Mf).tocsr()
        direct = D._lu(A).solve(b[free])
        out = R.P.pcg_classic(R.P.csr_apply(A), R.jacobi_apply(key, cK, cM)(np.float64), b[free], np.zeros(len(free), bool), iters=20000, rtol=rtol, stop=True)
        assert out.k_stop is not None
        err = R.rel(out.u[-1], direct)
        print("%s %s: converged PCG against splu %.2e" % (_name(key), name, err))
        assert err <= bar


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_floor_under_a_k_preconditioner_holds_for_the_first_iterations(key):
    """The device tests walk the loops under the two-level and multigrid preconditioners of K with the device hook as apply_M, so their floor can only
    be measured there (and is, per k). Its CPU stand-in, splu of K_ff as B in both walks, fixes the choice of k without a device: at k in HOOK_KS the
    gap is far below FLOOR_MAX on every mesh -- both starts of the Newmark pencil, and the COCG at the two highest frequencies, where Z is
    indefinite -- while at k = 8 it is not (1e-11 ... 7e-6 for the PCG). At the low frequencies the exact inverse is no stand-in: it solves Z x = f
    in one or two iterations and the later iterates are rounding, which the hierarchies, being approximate, do not do (measured on the device:
    <= 5e-13 at k = 8)."""
    kmax = max(R.HOOK_KS)
    b, x0 = R.newmark_rhs(key)
    cK, cM = R.newmark_pencils(key)["step"]
    worst8 = 0.0
    for start in (None, x0):
        ref = R.pcg_reference(key, cK, cM, b, start, R.proxy_apply(key), floor=R.TAU_HOOK)
        g = max(ref.gap_x[:kmax + 1].max(), ref.gap_s[:kmax + 1].max())
        worst8 = max(worst8, ref.gap_x.max(), ref.gap_s.max())
        print("%s pcg %s: floor up to k = %d %.2e, up to k = 8 %.2e" % (_name(key), "cold" if start is None else "warm", kmax, g, max(ref.gap_x.max(), ref.gap_s.max())))
        assert g <= 0.01 * R.FLOOR_MAX
    assert worst8 > R.FLOOR_MAX          # what the cut is for
    for case in H.CASES:
        for w in H.sweep_omegas(key)[3:]:
            zK, zM, cMj = R.harmonic_inputs(key, case, w)
            for kind in R.KINDS:
                ref = R.cocg_reference(key, zK, zM, cMj, H.load(key, kind), None, R.proxy_apply(key), floor=R.TAU_HOOK)
                g = max(ref.gap_x[:kmax + 1].max(), ref.gap_s[:kmax + 1].max())
                print("%s cocg %s omega %.4f %s: floor up to k = %d %.2e, up to k = 8 %.2e" % (_name(key), case, w, kind, kmax, g, max(ref.gap_x.max(), ref.gap_s.max())))
                assert g <= 0.1 * R.FLOOR_MAX


def test_the_stop_inputs_have_a_stop():
    """the inputs of the stop tests: pcg_iterates_util.exact_stop finds a k* within STOP_ITERS iterations of the block-Jacobi walks on both loops, and
    the floor holds up to there"""
    for key in U.SMALL:
        b, _ = R.newmark_rhs(key)
        cK, cM = R.newmark_pencils(key)["step"]
        zK, zM, cMj = R.harmonic_inputs(key, *R.stop_harmonic(key))
        for what, ref in (("pcg", R.pcg_reference(key, cK, cM, b, iters=R.STOP_ITERS)),
                          ("cocg", R.cocg_reference(key, zK, zM, cMj, H.load(key, "complex"), iters=R.STOP_ITERS))):
            ks, rtol = R.stop_rule(ref.res)
            print("%s %s: k* = %d, rtol %.3e, floor up to k* %.2e" % (_name(key), what, ks, rtol, ref.gap_x[:ks + 1].max()))
            assert 1 <= ks <= R.STOP_ITERS and 0 < rtol < 1
            assert ref.gap_x[:ks + 1].max() <= R.FLOOR_MAX and ref.gap_s[:ks + 1].max() <= R.FLOOR_MAX          # (tau of x_k* and of r.r at the stop)
