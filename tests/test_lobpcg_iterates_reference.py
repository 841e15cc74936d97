"""The reference recurrence of tests/lobpcg_iterates_util.py itself, on the CPU, for every input of tests/test_gpu_lobpcg_iterates.py that runs
under block-Jacobi (the inputs under a hierarchy take T from a device hook; their floors are asserted where they are measured):

  floors      the FP64 walk against the extended walk, in the measures the device is held to, stays within FLOOR_MAX at every k walked to
  pivots      the scaled Cholesky pivots of every basis stay above PIVOT_MIN = 1e-8, four decades above the loop's drop rule: no restart, no dropped
              column, and |W|, |P| are the same in both walks
  monotone    the Ritz values of the reference do not rise (Cauchy interlacing)
  truth       the extended walk, run on under block-Jacobi until the first nev residuals are below 1e-5, has the dense eigenvalues
              (modes_util.clamped_truth / free_truth, buckling_util.dense_truth, prestress_util.truth) to 1e-8: the reference is a correct LOBPCG,
              not merely a self-consistent one
  the stop    the threshold of each stop case keeps every reference residual up to the stop a factor 2 away, a column locks before the stop, and
              both walks stop at the same iteration

The floors printed here are the ones quoted in docs/design/04_12_modes.md, "Iterates pinned"."""
import numpy as np
import pytest
import scipy.linalg

import buckling_util as B
import lobpcg_iterates_util as LU
import modes_util as U
import prestress_util as PS

TRUTH_RTOL = 1e-5           # residual at which the long walk ends: the eigenvalue error is its square
TRUTH_ITERS = 1500


@pytest.mark.parametrize("case", LU.WALKED, ids=LU.case_name)
def test_floor_pivots_sets_and_monotone(case):
    ref = LU.jacobi_reference(case)
    kmax = max(case.ks)
    assert len(ref.lam) == kmax + 1 and ref.k_stop is None
    print("%s: m %d, floors at k <= %d: lam %.1e res %.1e subspace %.1e (FLOOR_MAX %.0e), smallest pivot %.1e, clusters %s" % (
        LU.case_name(case), ref.m, kmax, ref.gap_lam.max(), ref.gap_res.max(), ref.gap_sub.max(), LU.FLOOR_MAX, min(ref.pivots),
        [len(c) for c in LU.clusters(ref.lam[kmax])]))
    for name in ("gap_lam", "gap_res", "gap_sub"):
        g = getattr(ref, name)
        assert g.max() <= LU.FLOOR_MAX, "%s: %s %.2e at k = %d: replace this input" % (LU.case_name(case), name, g.max(), g.argmax())
    assert min(ref.pivots) >= LU.PIVOT_MIN, "a pivot of %.2e: the loop's rank decision is in doubt on this input" % min(ref.pivots)
    assert ref.restarts == 0 and ref.sets == ref.sets64
    for k in range(1, kmax + 1):
        want = (ref.m, ref.m if k > 1 else 0, 0)
        assert ref.sets[k] == want, "iteration %d: |W|, |P|, restarts = %s" % (k, ref.sets[k])
    assert LU.monotone_defect(ref.lam, 0.0) <= 1e-15


def _truth(case):
    """the dense eigenvalues the case's loop converges to"""
    p = LU.problem(case)
    if case.nq:          # the pencil restricted to the B-orthogonal complement of Q
        Bd = p.B.toarray()
        N = scipy.linalg.null_space((Bd @ p.Q).T)
        return scipy.linalg.eigh(N.T @ p.A.toarray() @ N, N.T @ Bd @ N, eigvals_only=True)
    if case.pencil == "buckling":
        return B.dense_truth(case.key, LU.prestress(case))[0]
    if case.pencil == "prestressed":
        return PS.truth(case.key, case.ratio)[0] / case.density
    if case.free:
        lam = U.free_truth(case.key)[0]
        return lam[(6 if p.bs == 3 else 3):] / case.density
    return U.clamped_truth(case.key)[0] / case.density


@pytest.mark.parametrize("case", LU.WALKED, ids=LU.case_name)
def test_extended_walk_converges_to_the_dense_truth(case):
    p = LU.problem(case)
    w = LU.walk(p, LU.jacobi_T(p), case.nev, TRUTH_ITERS, LU.XD, TRUTH_RTOL, keep=False)
    assert w.k_stop is not None, "no convergence within %d iterations (residuals %s)" % (TRUTH_ITERS, np.asarray(w.res[-1], dtype=float))
    lam = np.asarray(w.lam[-1][:case.nev], dtype=np.float64)
    want = _truth(case)[:case.nev]
    err = np.abs(lam - want).max() / np.abs(want).max()
    print("%s: %d iterations, eigenvalue error %.1e" % (LU.case_name(case), w.k_stop, err))
    assert err <= 1e-8
    assert LU.monotone_defect(w.lam, 0.0) <= 1e-15          # (the extended walk's own rounding, 1e-19, through the orthonormalisation)


@pytest.mark.parametrize("case", LU.STOP, ids=LU.case_name)
def test_stop_threshold_has_its_margin(case):
    rtol, ref = LU.jacobi_stop(case)
    k_stop, locked_before, margin = LU.stop_margin(ref, rtol)
    print("%s: rtol %.3g, k* %d, %d columns locked before it, margin %.2f; floors lam %.1e res %.1e subspace %.1e" % (
        LU.case_name(case), rtol, k_stop, locked_before, margin, ref.gap_lam.max(), ref.gap_res.max(), ref.gap_sub.max()))
    assert k_stop >= 1 and ref.k_stop64 == k_stop and locked_before >= 1 and margin >= 2.0
    assert max(ref.gap_lam.max(), ref.gap_res.max(), ref.gap_sub.max()) <= LU.FLOOR_MAX
    assert min(ref.pivots) >= LU.PIVOT_MIN and ref.restarts == 0 and ref.sets == ref.sets64
    locked = int((np.asarray(ref.res[0], dtype=float) <= rtol).sum())
    assert ref.sets[1][0] == ref.m - locked and 0 < locked < ref.m          # W holds the unconverged columns alone


def test_block_size_rule():
    assert [LU.block_size(nev, 10 ** 6) for nev in (1, 3, 4, 8, 20)] == [3, 5, 6, 10, 24]
    assert LU.block_size(2, 4) == 4
