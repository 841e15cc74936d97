"""The tall-skinny block kernels of mfh_modes against numpy, through their test hooks (host arrays in, host arrays out):
k_block_gram + its fixed-order second stage (G = A^T B) and k_block_update (Y = A C). Row counts: one row, the wave edge (63 / 64 / 65 rows;
64 is also the slab a workgroup of k_block_gram takes per step), several workgroups, and 100 003 rows -- more slabs than the kernel has
workgroups, with a ragged tail. Column counts: one column, counts below one 6 x 8 register tile, one past a tile edge against the full block,
and the full 24 x 24."""
import numpy as np
import pytest

import meshfem_amd as M

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ROWS = [1, 63, 64, 65, 1000, 100003]
COLS = [(1, 1), (3, 5), (7, 24), (24, 24)]


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def blocks():
    """One pair of random blocks per row count, shared by every column case (the leading columns are taken)."""
    rng = np.random.default_rng(11)
    out = {}
    for n in ROWS:
        A, B = np.asfortranarray(rng.standard_normal((n, 24))), np.asfortranarray(rng.standard_normal((n, 24)))
        # asymmetric in the columns and far from zero mean, so that a swapped index or a dropped slab shows
        A *= np.arange(1, 25)[None, :]
        B += 0.25
        A.setflags(write=False); B.setflags(write=False)
        out[n] = (A, B)
    return out


@pytest.mark.parametrize("pq", COLS, ids=lambda t: "p%d-q%d" % t)
@pytest.mark.parametrize("n", ROWS)
def test_block_gram(ctx, blocks, n, pq):
    """Every entry within n eps sum_i |a_i| |b_i| of the exact dot product -- the worst-case rounding bound of a length-n dot product in any
    summation order -- and two calls return the same bits (no atomics, fixed order of the partial sums)."""
    p, q = pq
    A, B = blocks[n][0][:, :p], blocks[n][1][:, :q]
    G = ctx.debug_block_gram(A, B)
    ref = np.array([[float(np.sum(A[:, i].astype(np.longdouble) * B[:, j].astype(np.longdouble))) for j in range(q)] for i in range(p)])
    bar = n * EPS * (np.abs(A).T @ np.abs(B))
    err = np.abs(G - ref)
    print("n %d p %d q %d: max error / bar %.3e" % (n, p, q, (err / bar).max()))
    assert G.shape == (p, q) and np.all(np.isfinite(G))
    assert np.all(err <= bar)
    assert np.array_equal(G, ctx.debug_block_gram(A, B))


@pytest.mark.parametrize("pq", COLS, ids=lambda t: "p%d-q%d" % t)
@pytest.mark.parametrize("n", ROWS)
def test_block_update(ctx, blocks, n, pq):
    """Y = A C: every entry within p eps sum_j |a_ij| |c_jk| of the exact value."""
    p, q = pq
    A = blocks[n][0][:, :p]
    Cm = np.random.default_rng(100 * p + q).standard_normal((p, q))
    Y = ctx.debug_block_update(A, Cm)
    ref = np.asarray(A.astype(np.longdouble) @ Cm.astype(np.longdouble), dtype=np.float64)
    bar = p * EPS * (np.abs(A) @ np.abs(Cm))
    err = np.abs(Y - ref)
    print("n %d p %d q %d: max error / bar %.3e" % (n, p, q, (err / np.maximum(bar, 1e-300)).max()))
    assert Y.shape == (n, q) and np.all(np.isfinite(Y))
    assert np.all(err <= bar)


def test_block_hooks_refuse_bad_shapes(ctx):
    from meshfem_amd import _lib
    A = np.zeros((8, 25), order="F")
    with pytest.raises(M.MeshFEMHipError) as ei:
        ctx.debug_block_gram(A, A[:, :3])
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(M.MeshFEMHipError) as ei:
        ctx.debug_block_update(A, np.zeros((25, 2)))
    assert ei.value.code == _lib.ERR_INVALID
