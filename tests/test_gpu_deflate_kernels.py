"""The projection kernels of mfh_modes_many against numpy, through their test hook (host arrays in, host arrays out): k_deflate_gram + its
fixed-order second stage (G = BQ^T V[:, cols]) and k_deflate_update (V[:, cols] -= Q G).
Row counts: those of tests/test_gpu_block_kernels.py -- one row, the wave edge (63 / 64 / 65; 64 is also the slab a workgroup of k_deflate_gram
takes per step), several workgroups, and 100 003 rows: more slabs than the kernel has workgroups along the rows, with a ragged tail.
Columns of Q: one; the 6-column tile of a wave and its neighbours (5, 6, 7); the widest count one workgroup takes at 24 / 16 / 8 columns of V
(24, 36, 72) and its neighbours -- a second workgroup along Q starts there; the cap 262; the unrolled-by-four loop of the update sees every
remainder. Columns of V: 1, 8, 9 (the 8-column tile edge and the 8 -> 16 accumulator variant of the update), 24; all of them, or a
non-contiguous list inside a 24-column block.
Bars (no measured number): a dot product of length n in any order errs by at most n eps sum |a_i| |b_i|; the update adds nq products to v, so its
error is at most (nq + 1) eps (|v| + sum |q_i| |c_i|)."""
import numpy as np
import pytest

import meshfem_amd as M

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ROWS = [1, 63, 64, 65, 1000, 100003]
NQ = [1, 5, 6, 7, 23, 24, 25, 35, 36, 37, 71, 72, 73, 262]
KS = [1, 8, 9, 24]
SPARSE = [0, 3, 23]                    # a non-contiguous column list


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    """One (BQ, Q, V) per row count, shared by every column case (the leading columns are taken)."""
    rng = np.random.default_rng(23)
    out = {}
    for n in ROWS:
        BQ = np.asfortranarray(rng.standard_normal((n, 262)))
        Q = np.asfortranarray(rng.standard_normal((n, 262)))
        V = np.asfortranarray(rng.standard_normal((n, 24)))
        # asymmetric in the columns and far from zero mean, so that a swapped index or a dropped slab shows
        BQ *= (1.0 + 0.01 * np.arange(262))[None, :]
        V += 0.25
        V *= np.arange(1, 25)[None, :]
        for a in (BQ, Q, V):
            a.setflags(write=False)
        out[n] = (BQ, Q, V)
    return out


def _cases():
    """Every nq at every k on the small row counts would be 300 cases; the edges are independent, so: all nq at k = 24 and at the sparse list for
    n = 65 and n = 1000, all k at the group edges 36 / 37, 72 / 73 and at the cap, and the other row counts at a few (nq, k)."""
    cases = []
    for n in (65, 1000):
        for nq in NQ:
            cases.append((n, nq, 24, None))
            cases.append((n, nq, 24, SPARSE))
        for k in KS:
            for nq in (36, 37, 72, 73, 262):
                cases.append((n, nq, k, None))
    for n in (1, 63, 64):
        for nq, k in ((1, 1), (7, 9), (73, 8), (262, 24)):
            cases.append((n, nq, k, None))
        cases.append((n, 25, 24, SPARSE))
    # (the extended-precision reference costs n nq k: the cap meets the long rows on the sparse list, 24 columns meet them at two groups of Q)
    for nq, k, cols in ((1, 1, None), (7, 24, None), (73, 8, None), (37, 9, None), (25, 24, None), (262, 24, SPARSE)):
        cases.append((100003, nq, k, cols))
    seen, uniq = set(), []
    for c in cases:
        key = (c[0], c[1], c[2], None if c[3] is None else tuple(c[3]))
        if key not in seen:
            seen.add(key)
            uniq.append(c)
    return uniq


def _id(c):
    return "n%d-nq%d-k%d-%s" % (c[0], c[1], c[2], "all" if c[3] is None else "sparse")


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_deflate(ctx, data, case):
    n, nq, nv, cols = case
    BQ, Q, V = data[n][0][:, :nq], data[n][1][:, :nq], data[n][2][:, :nv]
    cols = list(range(nv)) if cols is None else cols
    G, Vout = ctx.debug_deflate(BQ, Q, V, cols)
    Vc = V[:, cols]
    ld = np.longdouble
    ref = np.asarray(BQ.astype(ld).T @ Vc.astype(ld), dtype=np.float64)
    bar = n * EPS * (np.abs(BQ).T @ np.abs(Vc))
    err = np.abs(G - ref)
    print("gram   n %d nq %d k %d: max error / bar %.3e" % (n, nq, len(cols), (err / bar).max()))
    assert G.shape == (nq, len(cols)) and np.all(np.isfinite(G))
    assert np.all(err <= bar)
    # the update with the coefficients the device computed (C = G)
    uref = np.asarray(Vc.astype(ld) - Q.astype(ld) @ G.astype(ld), dtype=np.float64)
    ubar = (nq + 1) * EPS * (np.abs(Vc) + np.abs(Q) @ np.abs(G))
    uerr = np.abs(Vout[:, cols] - uref)
    print("update n %d nq %d k %d: max error / bar %.3e" % (n, nq, len(cols), (uerr / ubar).max()))
    assert Vout.shape == V.shape and np.all(np.isfinite(Vout))
    assert np.all(uerr <= ubar)
    # columns that are not listed are untouched, bit for bit
    rest = [j for j in range(nv) if j not in cols]
    assert np.array_equal(Vout[:, rest], V[:, rest])
    # repeats are bit-identical
    G2, V2 = ctx.debug_deflate(BQ, Q, V, cols)
    assert np.array_equal(G, G2) and np.array_equal(Vout, V2)


def test_column_order_follows_the_list(ctx, data):
    """A permuted list: column j of G belongs to V[:, cols[j]]."""
    n, nq = 1000, 25
    BQ, Q, V = data[n][0][:, :nq], data[n][1][:, :nq], data[n][2]
    cols = [17, 2, 9, 0]
    G, Vout = ctx.debug_deflate(BQ, Q, V, cols)
    Gs, Vs = ctx.debug_deflate(BQ, Q, V, sorted(cols))
    assert np.array_equal(G, Gs[:, [sorted(cols).index(c) for c in cols]])
    assert np.array_equal(Vout, Vs)


def test_deflate_hook_refuses_bad_shapes(ctx):
    from meshfem_amd import _lib
    Q = np.zeros((8, 263), order="F")
    V = np.zeros((8, 4), order="F")
    for call in (lambda: ctx.debug_deflate(Q, Q, V), lambda: ctx.debug_deflate(Q[:, :3], Q[:, :3], np.zeros((8, 25), order="F")),
                 lambda: ctx.debug_deflate(Q[:, :3], Q[:, :3], V, [0, 4]), lambda: ctx.debug_deflate(Q[:, :3], Q[:, :3], V, [1, 1]),
                 lambda: ctx.debug_deflate(Q[:, :3], Q[:, :3], V, [])):
        with pytest.raises(M.MeshFEMHipError) as ei:
            call()
        assert ei.value.code == _lib.ERR_INVALID
