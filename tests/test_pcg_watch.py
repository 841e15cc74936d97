"""The stopping rule of the PCG loops (ResidualWatch, mfh_solver.cpp), fed synthetic residual histories through mfh_debug_pcg_watch: one record
{r.r, p.Kp, "p.Kp is known"} per iteration. The rule: converged at the first r.r at or below the threshold; NaN, negative curvature at a complete
record, and a best r.r that has not dropped by 10 % within the stagnation window are reported as MFH_ERR_NOT_CONVERGED with a message. The last
record of a block of iterations is half-written (its p.Kp is not there yet) and Chronopoulos-Gear knows p.Kp only where alpha != 0: neither is
looked at. Window 0 switches the stagnation rule off (the multigrid batch and the classic partitioned loop run without it). No GPU needed."""
import ctypes as C

import numpy as np
import pytest

OK = 0


def _status_not_converged():
    # MFH_ERR_NOT_CONVERGED from the header, so that the test does not carry a copy of the number
    import os
    import re
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(here, "include", "meshfem_hip.h")).read()
    m = re.search(r"MFH_ERR_NOT_CONVERGED\s*=\s*(-?\d+)", text)
    assert m, "MFH_ERR_NOT_CONVERGED not found in meshfem_hip.h"
    return int(m.group(1))


def watch(rr, threshold, window=0, pkp=None, known=None, last_complete=None):
    """-> (status, convergedAt, message)"""
    from meshfem_amd._lib import load
    lib = load()
    rr = np.ascontiguousarray(rr, dtype=np.float64)
    n = len(rr)
    pkp = np.ones(n) if pkp is None else np.ascontiguousarray(pkp, dtype=np.float64)
    known = np.ones(n, dtype=np.uint8) if known is None else np.ascontiguousarray(known, dtype=np.uint8)
    if last_complete is None:
        last_complete = n - 1
    at = C.c_int64(-7)
    msg = C.create_string_buffer(512)
    st = lib.mfh_debug_pcg_watch(n, rr.ctypes.data, pkp.ctypes.data, known.ctypes.data, float(threshold), int(window), int(last_complete), C.byref(at),
                                 msg, len(msg))
    return st, at.value, msg.value.decode()


def test_converges_at_the_first_record_at_or_below_the_threshold_and_not_before():
    rr = [1.0, 0.5, 0.2, 0.1 + 1e-12, 0.1, 0.05, 0.2, 0.01]
    assert watch(rr, 0.1) == (OK, 4, "")                    # equality counts (rr <= threshold); 0.1 + 1e-12 does not
    assert watch(rr[:4], 0.1) == (OK, -1, "")               # not yet
    assert watch(rr, 1.0) == (OK, 0, "")                    # the start residual already meets it
    assert watch([0.0, 0.0], 0.0) == (OK, 0, "")            # a zero right-hand side: 0 <= 0
    assert watch([], 0.1) == (OK, -1, "")


def test_nan_residual_is_a_breakdown():
    st, at, msg = watch([1.0, 0.5, float("nan"), 1e-9], 1e-6)
    assert st == _status_not_converged() and at == -1
    assert msg == "PCG breakdown (NaN residual): K is not SPD on the free variables"
    # a record at or below the threshold ends the scan: what follows it is not looked at
    assert watch([1.0, 1e-9, float("nan")], 1e-6) == (OK, 1, "")


def test_negative_curvature_at_a_complete_record_only():
    rr = [1.0, 0.8, 0.6, 0.4]
    pkp = [2.0, 1.0, -0.25, 1.0]
    st, at, msg = watch(rr, 1e-6, pkp=pkp)
    assert st == _status_not_converged() and at == -1
    assert msg == "PCG breakdown (p.Kp = -0.250000 < 0 at iteration 2, residual^2 0.600000): K is not positive definite on the free variables"
    # the same value in the half-written last record of a block is not looked at ...
    assert watch(rr[:3], 1e-6, pkp=pkp[:3], last_complete=1) == (OK, -1, "")
    # ... nor where the loop does not know p.Kp (Chronopoulos-Gear: alpha == 0)
    assert watch(rr, 1e-6, pkp=pkp, known=[1, 1, 0, 1]) == (OK, -1, "")
    # zero curvature is not negative; convergence is judged before the curvature of the same record
    assert watch(rr, 1e-6, pkp=[2.0, 0.0, 0.0, 1.0]) == (OK, -1, "")
    assert watch([1.0, 1e-9], 1e-6, pkp=[1.0, -1.0]) == (OK, 1, "")


def test_a_plateau_shorter_than_the_window_followed_by_progress_is_not_an_error():
    # the case the window was sized for: block-Jacobi PCG on a one-layer plate in bending, 59 k DoF, sits above its best residual for more than
    # 5 000 iterations and converges at 5 913. Its window is max(max(5000, 40 check_every), min(n, 50000)) = 50 000 iterations.
    rr = np.concatenate([np.geomspace(1.0, 1e-3, 400), np.full(5400, 2e-3), np.geomspace(2e-3, 1e-13, 114)])
    assert len(rr) == 5914
    assert watch(rr, 1.1e-13, window=50000) == (OK, 5913, "")
    # with the 5 000 iterations a small system gets, the same history is a stagnation
    st, at, msg = watch(rr, 1.1e-13, window=5000)
    assert st == _status_not_converged() and at == -1 and msg.startswith("PCG stagnated (no progress of the residual for 5000 iterations)")


def test_a_plateau_longer_than_the_window_is_reported_at_its_end():
    rr = np.concatenate([[1.0, 0.5], np.full(100, 0.5)])          # best at record 1
    st, at, msg = watch(rr, 1e-6, window=50)
    assert st == _status_not_converged() and at == -1
    assert msg == ("PCG stagnated (no progress of the residual for 50 iterations): the system is singular with an inconsistent right-hand side "
                   "(missing boundary conditions?) or too ill-conditioned for this preconditioner")
    # reported at the first record MORE than `window` after the best one: 1 + 50 records pass, record 52 does not
    assert watch(rr[:52], 1e-6, window=50) == (OK, -1, "")
    assert watch(rr[:53], 1e-6, window=50)[0] == _status_not_converged()


def test_window_zero_never_reports_stagnation():
    rr = np.full(200000, 0.5)
    assert watch(rr, 1e-6, window=0) == (OK, -1, "")
    assert watch(np.concatenate([rr, [1e-7]]), 1e-6, window=0) == (OK, 200000, "")


@pytest.mark.parametrize("factor,stagnates", [(0.9, True), (np.nextafter(0.9, 0.0), False), (0.95, True), (0.5, False)])
def test_only_a_residual_below_nine_tenths_of_the_best_counts_as_progress(factor, stagnates):
    # best = 1 at record 0; every later record is factor * 1. The rule is rr < 0.9 best, strictly: 0.9 itself is no progress.
    # (with progress each record becomes the new best, and the following ones at the same value are then a plateau of their own: keep it short)
    window = 10
    rr = np.concatenate([[1.0], np.full(window + 1, factor)])
    st, at, _ = watch(rr, 1e-6, window=window)
    assert at == -1
    assert (st == _status_not_converged()) == stagnates
