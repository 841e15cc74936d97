"""The reference recurrences of tests/pcg_iterates_util.py against what does not depend on them, on the meshes of
tests/test_gpu_pcg_iterates.py (3D 4 x 3 x 3 tets, 2D 20 x 16 quads, interior vertices moved by 4 %; P2 and P1 elasticity with the
isotropic field, the scalar P2 Laplacian; the face x = min fixed), block-Jacobi from the oracle's K:

- the classic recurrences converge to the dense direct solution of the lifted system (non-zero fixed values included);
- the Chronopoulos-Gear form walks the same iterates: 12 iterations to 1e-13;
- FP64 vectors and longdouble vectors (dot products in longdouble both times) agree to 1e-14 over 12 iterations, in both forms: the
  rounding floor under the 1e-12 of the GPU tests. Observed maxima over the five problems (x86-64 longdouble, 64-bit mantissa):
  classic 6.1e-16, Chronopoulos-Gear 4.2e-15 (3D P1); FP64 dot products instead of longdouble ones: 6.7e-16; classic against
  Chronopoulos-Gear in FP64: 4.1e-15;
- the two-eigenvector right-hand side converges at exactly iteration 2, relative residual <= 1e-12 (observed 5.1e-16 .. 5.2e-15)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import pcg_iterates_util as P

PROBLEMS = [(3, 2, "elasticity"), (3, 1, "elasticity"), (2, 2, "elasticity"), (2, 1, "elasticity"), (3, 2, "laplacian")]
_CACHE = {}


def _problem(dim, deg, op):
    """(K, block size, fixed mask, f, ubar): built once per problem and left unchanged."""
    key = (dim, deg, op)
    if key not in _CACHE:
        from oracle import meshfem_oracle as O
        V, T = P.mesh(dim)
        m = O.FEMMesh(T, V, deg)
        if op == "laplacian":
            K, bs = P.oracle_laplacian(T, V, deg)[0], 1
        else:
            K, bs = P.oracle_K(dim, deg, m.elem_nodes, V, P.iso_field(dim, len(T))[2], m.num_nodes), dim
        nodes = np.nonzero(m.node_pos[:, 0] < V[:, 0].min() + 1e-9)[0]
        fixed = np.zeros(K.shape[0], bool)
        fixed[(nodes[:, None] * bs + np.arange(bs)).ravel()] = True
        rng = np.random.default_rng(31)
        f = rng.standard_normal(K.shape[0])
        ubar = np.where(fixed, 0.01 * rng.standard_normal(K.shape[0]), 0.0)
        _CACHE[key] = (K, bs, fixed, f, ubar)
    return _CACHE[key]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("dim,deg,op", PROBLEMS)
def test_classic_reference_converges_to_the_direct_solution(dim, deg, op):
    K, bs, fixed, f, ubar = _problem(dim, deg, op)
    free = ~fixed
    u = ubar.copy()
    u[free] = spla.spsolve(sp.csc_matrix(K[free][:, free]), (f - K @ ubar)[free])
    ref = P.pcg_classic(P.csr_apply(K), P.block_jacobi_apply(K, bs, fixed), f, fixed, ubar, iters=1500, rtol=1e-13, stop=True)
    assert ref.k_stop is not None, ref.res[-1]
    got = ref.u[ref.k_stop]
    assert np.array_equal(got[fixed], ubar[fixed])
    # |x - x*| <= cond(M^-1 K) x the relative residual: well inside 1e-9 at 1e-13
    assert _rel(got, u) <= 1e-9, _rel(got, u)
    assert ref.res[0] == 1.0 and np.array_equal(ref.u[0], ubar)


@pytest.mark.parametrize("dim,deg,op", PROBLEMS)
def test_rounding_floor_and_the_two_forms(dim, deg, op, capsys):
    K, bs, fixed, f, ubar = _problem(dim, deg, op)
    LD = np.longdouble
    runs = {}
    for form, fn in (("classic", P.pcg_classic), ("cg", P.pcg_chronopoulos_gear)):
        runs[form, "f64"] = fn(P.csr_apply(K), P.block_jacobi_apply(K, bs, fixed), f, fixed, ubar, iters=12)
        runs[form, "ld"] = fn(P.csr_apply(K, LD), P.block_jacobi_apply(K, bs, fixed), f, fixed, ubar, iters=12, dtype=LD)
    runs["classic", "dot64"] = P.pcg_classic(P.csr_apply(K), P.block_jacobi_apply(K, bs, fixed), f, fixed, ubar, iters=12, dot=P.dot_fp64)

    def worst(a, b):
        return max(_rel(runs[a].u[k], runs[b].u[k]) for k in range(1, 13))
    floor = {form: worst((form, "f64"), (form, "ld")) for form in ("classic", "cg")}
    forms = worst(("cg", "f64"), ("classic", "f64"))
    dots = worst(("classic", "dot64"), ("classic", "f64"))
    with capsys.disabled():
        print("\n%dD P%d %s: FP64 vs longdouble classic %.2e, Chronopoulos-Gear %.2e; the two forms %.2e; FP64 dots %.2e"
              % (dim, deg, op, floor["classic"], floor["cg"], forms, dots))
    assert floor["classic"] <= 1e-14 and floor["cg"] <= 1e-14, floor
    # two orders of rounding errors of the same walk: ten floors
    assert forms <= 1e-13, forms
    res = np.abs(runs["cg", "f64"].res / runs["classic", "f64"].res - 1.0).max()
    assert res <= 1e-13, res


@pytest.mark.parametrize("dim,deg,op", PROBLEMS)
def test_two_eigenvector_rhs_converges_at_iteration_two(dim, deg, op, capsys):
    K, bs, fixed, _, _ = _problem(dim, deg, op)
    b = P.two_eigenvector_rhs(K, bs, fixed)
    assert np.all(b[fixed] == 0.0)
    for fn in (P.pcg_classic, P.pcg_chronopoulos_gear):
        ref = fn(P.csr_apply(K), P.block_jacobi_apply(K, bs, fixed), b, fixed, iters=3, rtol=1e-12)
        with capsys.disabled():
            print("\n%dD P%d %s %s: residuals %s" % (dim, deg, op, fn.__name__, ref.res))
        assert ref.k_stop == 2, ref.res
        assert ref.res[1] > 1e-3, ref.res                  # not a one-vector right-hand side
        assert ref.res[2] <= 1e-12, ref.res


def test_exact_stop_picks_a_rounding_proof_threshold():
    res = np.array([1.0, 0.95, 1.2, 0.5, 0.49, 0.1])
    k, rtol = P.exact_stop(res)
    assert k == 3 and rtol == pytest.approx(np.sqrt(0.5 * 0.95))
    assert res[k] < rtol < min(res[:k])


def test_zero_right_hand_side_returns_the_fixed_values():
    K, bs, fixed, f, ubar = _problem(2, 1, "elasticity")
    ref = P.pcg_classic(P.csr_apply(K), P.block_jacobi_apply(K, bs, fixed), np.zeros(len(f)), fixed, iters=3, rtol=1e-8)
    assert ref.k_stop == 0 and all(np.all(u == 0.0) for u in ref.u)
