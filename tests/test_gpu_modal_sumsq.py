"""k_modal_sumsq alone, through its hook (mfh_debug_modal_sumsq): out[row] = sum_t (sum_j B_j[row] F[j][t])^2, the inner sums fma chains over the
columns j ascending from +0, the outer one fma(s_t, s_t, acc) over t ascending from +0, optionally the square root. Shapes: k_modal_expand's -- row
counts with tails and an odd one, column counts around the unroll of four and the largest (258), ranks around the columns per pass NP, and with five
columns 2 048 x 256 + 257 rows, where alone lanes take a second trip of the grid-stride loop. Random B and F with a few exact zeros, one column of
scale 1e+100 against a coefficient row of 1e-100 and one the other way round (the squares halve the exponent range the expansion kernel's test uses).
  accuracy     against long double within modal_random_util.sumsq_prefixes' bound of the fma chains, with and without the root
  grouping     1, 8, 16 and 32 columns of F per pass (all three instantiations; passes that read the accumulator back): identical bits
  column list  factors of mfh_psd_factor's form with their pivots: the later passes leave the earlier pivots' columns out; the bits of the full lists
  determinism  two calls: identical bits
  rank 0       zeros, B (all NaN here) is not read."""
import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import _lib

import modal_random_util as R
import modal_util as MU

pytestmark = pytest.mark.gpu

NP = MU.NP_DEFAULT
ROWS = [1, 63, 64, 65, 257, 1000, 70001]
STRIDE_ROWS = 2048 * 256 + 257      # more rows than the capped grid has lanes
COLS = [1, 3, 4, 5, 7, 258]
RANKS = [1, 2, NP - 1, NP, NP + 1, 2 * NP + 3]


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def _inputs(n, nb):
    rng = np.random.default_rng(2000 * nb + n % 997)
    B = rng.standard_normal((nb, n))
    F = rng.standard_normal((nb, RANKS[-1]))
    B[rng.integers(0, nb, 8), rng.integers(0, n, 8)] = 0.0
    F[rng.integers(0, nb, 4), rng.integers(0, RANKS[-1], 4)] = 0.0
    B[0] *= 1e100
    F[0] *= 1e-100
    if nb > 1:
        B[nb - 1] *= 1e-100
        F[nb - 1] *= 1e100
    return B, F


@pytest.mark.parametrize("n,nb", [(n, nb) for n in ROWS for nb in COLS] + [(STRIDE_ROWS, 5)])
def test_sumsq(ctx, n, nb):
    c = ctx
    B, F = _inputs(n, nb)
    refs = R.sumsq_prefixes(B, F, RANKS)
    worst = 0.0
    for r in RANKS:
        Fr = np.ascontiguousarray(F[:, :r])
        out = c.debug_modal_sumsq(B, Fr)
        ref, bound, root_ref, root_bound = refs[r]
        err = np.abs((out - ref).astype(np.float64))
        worst = max(worst, float((err / bound).max()))
        assert out.shape == (n,) and np.all(np.isfinite(out)) and np.all(out >= 0.0)
        assert np.all(err <= bound)
        rt = c.debug_modal_sumsq(B, Fr, sqrt=True)
        assert np.all(np.abs((rt - root_ref).astype(np.float64)) <= root_bound)
        assert np.array_equal(rt, np.sqrt(out))              # the root is the correctly rounded root of the stored sum
        for ppp in (1, 8, 16):
            if ppp == 1 and (r > NP + 1 or n > 1000):
                continue
            assert np.array_equal(c.debug_modal_sumsq(B, Fr, planes_per_pass=ppp), out), "columns per pass %d" % ppp
    assert np.array_equal(c.debug_modal_sumsq(B, Fr), out)
    print("n %d nb %d: worst error / bound %.3e" % (n, nb, worst))


@pytest.mark.parametrize("n,nb,rank,ppp", [(1000, 7, 7, 2), (257, 33, 20, 8), (70001, 258, 70, 16), (1000, 258, 258, 32), (65, 40, 40, 1)])
def test_column_lists_change_no_bit(ctx, n, nb, rank, ppp):
    """F and piv from the twin of mfh_psd_factor: row piv[s] of F is exactly zero after column s, so the pass that begins at column t0 may leave out
    the columns piv[0 .. t0) of the basis."""
    c = ctx
    rng = np.random.default_rng(n + nb)
    A = rng.standard_normal((nb, rank))
    F, piv, _ = R.psd_factor_twin(A @ A.T)
    B = rng.standard_normal((nb, n))
    full = c.debug_modal_sumsq(B, F, planes_per_pass=ppp)
    assert np.array_equal(c.debug_modal_sumsq(B, F, piv=piv, planes_per_pass=ppp), full)
    assert np.array_equal(c.debug_modal_sumsq(B, F, piv=piv), full)
    ref, bound = R.sumsq_prefixes(B, F, [F.shape[1]])[F.shape[1]][:2]
    assert np.all(np.abs((full - ref).astype(np.float64)) <= bound)
    # a list that would leave out a non-zero coefficient is refused, not run
    if F.shape[1] > ppp:
        bad = F.copy()
        bad[piv[0], -1] = 1.0
        with pytest.raises(M.MeshFEMHipError) as ei:
            c.debug_modal_sumsq(B, bad, piv=piv, planes_per_pass=ppp)
        assert ei.value.code == _lib.ERR_INVALID


def test_rank_zero_and_refusals(ctx):
    c = ctx
    out = c.debug_modal_sumsq(np.full((5, 300), np.nan), np.zeros((5, 0)))
    assert out.shape == (300,) and np.all(out == 0.0)
    assert np.all(c.debug_modal_sumsq(np.full((5, 300), np.nan), np.zeros((5, 0)), sqrt=True) == 0.0)
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.debug_modal_sumsq(np.zeros((259, 4)), np.zeros((259, 2)))
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.debug_modal_sumsq(np.zeros((3, 4)), np.zeros((3, 2)), planes_per_pass=33)
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.debug_modal_sumsq(np.zeros((3, 4)), np.zeros((3, 2)), piv=[0, 3])
    assert ei.value.code == _lib.ERR_INVALID
