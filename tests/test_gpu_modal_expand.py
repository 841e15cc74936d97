"""The kernels of mfh_modal.hip alone, through their debug hooks.
k_modal_expand (mfh_debug_modal_expand): out[p][row] = sum_j B_j[row] C[j][p] as the fma chain over j ascending from +0. Shapes: row counts with
tails and an odd one; column counts around the kernel's unroll of four and the largest (258); plane counts around the planes per pass NP; and, with
five columns, 2 048 x 256 + 257 rows: the grid is capped at 2 048 workgroups of 256 lanes, so only there do lanes take a second trip of the
grid-stride loop (the first 257 rows two trips, the rest one). Random B and C with a few exact zeros, one column of scale 1e+150 against a
coefficient row of 1e-150 and one the other way round.
  accuracy     against B^T C in long double, componentwise: |err| <= (nb + 1) eps sum_j |B_j| |C_j|, the gamma bound of a chain of nb fmas
  grouping     the same planes written 1, NP and the default number per pass: identical bits
  determinism  two calls: identical bits
The long-double reference of a (n, nb) pair is computed once for the largest plane count; the smaller counts take its leading planes (the value of
a plane does not depend on the others).
k_modal_gram + k_modal_gram_sum (mfh_debug_modal_gram): G = A^T V against long double within (n + 1) eps sum_rows |A_i| |V_j| (any order of the n
terms), two calls identical bits; column counts around the tile of 8, and row counts beyond 256 x 256, where its lanes loop."""
import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import _lib

import modal_util as MU

pytestmark = pytest.mark.gpu

NP = MU.NP_DEFAULT
ROWS = [1, 63, 64, 65, 257, 1000, 70001]
STRIDE_ROWS = 2048 * 256 + 257      # more rows than the capped grid has lanes
COLS = [1, 3, 4, 5, 7, 258]
PLANES = [1, 2, NP - 1, NP, NP + 1, 2 * NP + 3]


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def _inputs(n, nb):
    rng = np.random.default_rng(1000 * nb + n % 997)
    B = rng.standard_normal((nb, n))
    C = rng.standard_normal((nb, PLANES[-1]))
    B[rng.integers(0, nb, 8), rng.integers(0, n, 8)] = 0.0
    C[rng.integers(0, nb, 4), rng.integers(0, PLANES[-1], 4)] = 0.0
    B[0] *= 1e150
    C[0] *= 1e-150
    if nb > 1:
        B[nb - 1] *= 1e-150
        C[nb - 1] *= 1e150
    return B, C


def _reference(B, C):
    """(B^T C)^T in long double: [nPlanes, n] (numpy's own loop over j ascending: 3 s for the largest shape)."""
    return (np.ascontiguousarray(B.T.astype(np.longdouble)) @ C.astype(np.longdouble)).T


@pytest.mark.parametrize("n,nb", [(n, nb) for n in ROWS for nb in COLS] + [(STRIDE_ROWS, 5)])
def test_expand(ctx, n, nb):
    c = ctx
    B, C = _inputs(n, nb)
    ref, bound = _reference(B, C), MU.expand_bound(B, C)
    worst = 0.0
    for planes in PLANES:
        Cp = np.ascontiguousarray(C[:, :planes])
        out = c.debug_modal_expand(B, Cp)
        assert out.shape == (planes, n)
        err = np.abs((out - ref[:planes]).astype(np.float64))
        worst = max(worst, float((err / np.maximum(bound[:planes], np.finfo(float).tiny)).max()))
        assert np.all(err <= bound[:planes])
        for ppp in (1, NP):
            assert np.array_equal(c.debug_modal_expand(B, Cp, planes_per_pass=ppp), out), "planes per pass %d" % ppp
    assert np.array_equal(c.debug_modal_expand(B, Cp), out)
    print("n %d nb %d: worst error / bound %.3e" % (n, nb, worst))


def test_refusals(ctx):
    c = ctx
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.debug_modal_expand(np.zeros((259, 4)), np.zeros((259, 2)))
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.debug_modal_expand(np.zeros((3, 4)), np.zeros((3, 2)), planes_per_pass=33)
    assert ei.value.code == _lib.ERR_INVALID


@pytest.mark.parametrize("n", [1, 255, 257, 70001, 256 * 256 * 2 + 77])
def test_gram(ctx, n):
    """70 001 rows: the row blocks exceed the cap of 256 workgroups, so the lanes loop (twice for most of them at the largest count)."""
    c = ctx
    rng = np.random.default_rng(n)
    for na, nv in ((1, 1), (7, 2), (8, 8), (9, 3), (258, 8)) if n <= 70001 else ((9, 3),):
        A, V = rng.standard_normal((na, n)), rng.standard_normal((nv, n))
        A[0, 0] = 0.0
        G = c.debug_modal_gram(A, V)
        ref = A.astype(np.longdouble) @ V.astype(np.longdouble).T
        bound = MU.gram_bound(A, V)
        err = np.abs((G - ref).astype(np.float64))
        assert G.shape == (na, nv) and np.all(err <= bound), (na, nv, (err / bound).max())
        assert np.array_equal(c.debug_modal_gram(A, V), G)
