"""The four PCG loops of the library (solve_one_classic, solve_cg, solve_multigrid_batch; solve_classic_partitioned in
test_gpu_pcg_iterates_distributed.py) and their vector kernels, ITERATE BY ITERATE against the plain reference recurrences of
tests/pcg_iterates_util.py: with rtol = 1e-30 and maxit = k the library returns x_k + ubar (and the status "not converged", which the
Python wrappers turn into an exception before they return u: the helper below calls the C entry as core.py does and accepts exactly
that status). A converged solution forgives a wrong beta, a stale alpha or an x that moves after convergence; an iterate does not.

What is pinned (every element type the row applies to: P2 / P1 elasticity in 3D and 2D, the scalar P2 Laplacian for the DIM = 1
kernels; P2 on the cluster operator, P1 and the Laplacian on the assembled SpMV, one P2 case assembled), each at k in {1, 2, 3, 5, 8},
eager (pcg_graph 0) and in one captured block (check_every = k):

    loop                                                      reached by                              apply_M of the reference
    classic, block-Jacobi (k_pcg_init/update/direction)       pcg_variant 0                           oracle K's inverse diagonal blocks
    classic, two-level (SKIPZ, r.z from k_tl_apply)           PRECOND_TWO_LEVEL                       debug_apply_precond
    classic, multigrid unfused (k_mg_rz)                      mg_fuse 0                               debug_apply_precond
    classic, multigrid fused (ZS, k_mg_cheb_rz)               mg_fuse 1, mg_dinv_fp32 0               debug_apply_precond
    the same with the FP32 Dinv copy                          defaults                                debug_apply_precond (FP64 map)
    classic under deterministic 1 (commit_sums, k_det_finish) block-Jacobi and multigrid              as above
    Chronopoulos-Gear, one vector (k_cg_init, k_cg_update1)   pcg_variant 1; block-Jacobi, two-level  as above
    Chronopoulos-Gear, batches 2, 6 (3D), 3 (2D) (k_cg_update) batch_rhs 1, mfh_solve_batch           as above
    multigrid batch (solve_multigrid_batch), P2 only          mg_batch 1                              debug_apply_precond

Bounds: |u - u_k| <= tau |u_k| with tau = 1e-12 where apply_M comes from the oracle (Y_RTOL of the operator tests; the reference's own
rounding floor is 4e-15, tests/test_pcg_iterates_reference.py) and 1e-11 where it is the hook (HIP_RTOL of test_shape_derivatives.py:
the hook's launch and the loop's own are separate sums); rel_residual to 10 tau, true_rel_residual to 1e-9, the fixed rows bit for bit.
With the FP32 copy of the smoother's inverse blocks the loop runs ANOTHER preconditioner than the hook's (one rounding of 2^-24 per
block entry): the iterate is compared at 1e-5 there, and the residuals, which must not depend on M being the hook's map, are compared at
their bounds with |mask(f - K u)| / |b| of the RETURNED iterate, formed on the host with the oracle's K. Measured deviation of the
iterate from the FP64 map's: see the design note (docs/design/04_5_pcg_vector_kernels.md, "Iterates pinned").

Then the exact stop (k* where the reference residual first falls 10 % below every earlier one, rtol the geometric mean: every loop
reports converged at k* and returns x_k*, also from inside a captured block of 8 that runs past k* behind closed gates; bit for bit
between eager and graph under deterministic 1), per-vector control in batches (a scaled copy, a zero vector, a right-hand side that
freezes at iteration 2 while its mates run on), and the kernels past their grid caps."""
import time

import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import _lib as L
from meshfem_amd._lib import ptr
import pcg_iterates_util as P

pytestmark = pytest.mark.gpu

TAU_ORACLE = 1e-12
TAU_HOOK = 1e-11
TAU_FP32_ITERATE = 1e-5
KS = (1, 2, 3, 5, 8)
DEFAULTS = dict(pcg_variant=-1, batch_rhs=0, mg_batch=1, mg_fuse=1, mg_dinv_fp32=1, pcg_graph=1, check_every=50)

# (dim, deg, operator, boundary condition)
CASES = [(3, 2, "elasticity", "zero"), (3, 1, "elasticity", "zero"), (2, 2, "elasticity", "zero"), (2, 1, "elasticity", "zero"),
         (3, 2, "laplacian", "zero"), (3, 2, "elasticity", "nonzero"), (2, 2, "elasticity", "periodic"), (3, 2, "assembled", "zero")]

# name -> (context options before the mesh, preconditioner, solve options, batched, apply_M, tau of the iterate)
BJ, TL, MG = M.PRECOND_BLOCK_JACOBI, M.PRECOND_TWO_LEVEL, M.PRECOND_MULTIGRID
LOOPS = {
    "classic_bj": ((), BJ, dict(pcg_variant=0), False, "oracle", TAU_ORACLE),
    "classic_tl": ((), TL, dict(pcg_variant=0), False, "hook", TAU_HOOK),
    "classic_mg_unfused": ((), MG, dict(pcg_variant=0, mg_fuse=0), False, "hook", TAU_HOOK),
    "classic_mg_fused": ((), MG, dict(pcg_variant=0, mg_fuse=1, mg_dinv_fp32=0), False, "hook", TAU_HOOK),
    "classic_mg_fused_fp32": ((), MG, dict(pcg_variant=0), False, "hook", TAU_FP32_ITERATE),
    "det_bj": ((("deterministic", 1),), BJ, dict(), False, "oracle", TAU_ORACLE),
    "det_mg": ((("deterministic", 1),), MG, dict(mg_dinv_fp32=0), False, "hook", TAU_HOOK),
    "cg_bj": ((), BJ, dict(pcg_variant=1), False, "oracle", TAU_ORACLE),
    "cg_tl": ((), TL, dict(pcg_variant=1), False, "hook", TAU_HOOK),
    "cgbatch_bj": ((), BJ, dict(pcg_variant=1, batch_rhs=1), True, "oracle", TAU_ORACLE),
    "cgbatch_tl": ((), TL, dict(pcg_variant=1, batch_rhs=1), True, "hook", TAU_HOOK),
    "mgbatch_unfused": ((), MG, dict(mg_batch=1, mg_fuse=0), True, "hook", TAU_HOOK),
    "mgbatch_fused": ((), MG, dict(mg_batch=1, mg_fuse=1, mg_dinv_fp32=0), True, "hook", TAU_HOOK),
    "mgbatch_fused_fp32": ((), MG, dict(mg_batch=1), True, "hook", TAU_FP32_ITERATE),
}
BATCHES = {3: (2, 6), 2: (3,), 1: (2, 3, 6)}        # by block size


def _applies(case, loop):
    dim, deg, op, bc = case
    if op == "assembled":
        return loop in ("classic_bj", "classic_mg_unfused", "cg_bj", "cgbatch_bj")
    if op == "laplacian":
        return loop in ("classic_bj", "det_bj", "cg_bj", "cgbatch_bj")
    if loop.startswith("mgbatch"):
        return deg == 2 and op == "elasticity"
    return True


GRID = [(c, l) for c in CASES for l in LOOPS if _applies(c, l)]
_IDS = ["%dD-P%d-%s-%s-%s" % (c + (l,)) for c, l in GRID]

_PROBLEMS = {}


class _Problem:
    """One case: the mesh, the oracle's K, the fixed rows and their values, eight right-hand sides -- computed once, left unchanged."""

    def __init__(self, case):
        dim, deg, op, bc = case
        self.case, self.dim, self.deg, self.op, self.bc = case, dim, deg, op, bc
        self.V, self.T = P.mesh(dim)
        self.E, self.nu, D = P.iso_field(dim, len(self.T))
        c = self.context()
        try:
            self.n_dof = c.n_dof
            pos = c.node_positions()
            if bc == "periodic":
                dof = c.get_dof_map()[0]
                dofs = np.array([dof[c.pin_node()]])
            else:
                dof = None
                dofs = np.unique(np.nonzero(pos[:, 0] < self.V[:, 0].min() + 1e-9)[0])
            if op == "laplacian":
                self.bs = 1
                self.K, m = P.oracle_laplacian(self.T, self.V, deg)
                assert np.array_equal(m.elem_nodes, c.elem_nodes())
            else:
                self.bs = dim
                self.K = P.oracle_K(dim, deg, c.elem_nodes(), self.V, D, c.n_dof, dof)
        finally:
            c.close()
        n = self.bs * self.n_dof
        assert self.K.shape == (n, n)
        self.vars = (dofs[:, None] * self.bs + np.arange(self.bs)).ravel()
        self.fixed = np.zeros(n, bool)
        self.fixed[self.vars] = True
        rng = np.random.default_rng(41)
        self.ubar = np.zeros(n)
        if bc == "nonzero":
            self.ubar[self.vars] = 0.01 * rng.standard_normal(len(self.vars))
        self.F = rng.standard_normal((8, n))
        self.apply_K = P.csr_apply(self.K)
        self.bj = P.block_jacobi_apply(self.K, self.bs, self.fixed)
        self._refs = {}
        self._eig = None

    def context(self, pre=()):
        c = M.Context(0)
        for k, v in pre:
            c.set_option(k, v)
        if self.deg == 1 or self.op != "elasticity":          # P1, the scalar operator and the assembled P2 case: the assembled SpMV, both triangles
            c.set_option("matrix_free", 0)
            c.set_option("matrix_storage", 0)
        c.mesh_build(self.T, self.V, self.deg)
        if self.op == "laplacian":
            c.set_operator(M.OP_LAPLACIAN)
        else:
            c.material_iso_field(self.E, self.nu)
        if self.bc == "periodic":
            c.apply_periodic_conditions()
        if hasattr(self, "vars"):
            c.fix_variables(self.vars, self.ubar[self.vars])
            info = c.matrix_free_info()
            assert info["active"] == (self.deg == 2 and self.op == "elasticity"), info
            if info["active"]:
                assert info["mode"] == 4, info
        return c

    def eig_rhs(self):
        if self._eig is None:
            self._eig = P.two_eigenvector_rhs(self.K, self.bs, self.fixed)
        return self._eig

    def reference(self, f, apply_M, key=None, iters=8):
        """the classic reference walk for one right-hand side; block-Jacobi walks (key given) are shared between the tests"""
        if key is not None and key in self._refs:
            return self._refs[key]
        ref = P.pcg_classic(self.apply_K, apply_M, f, self.fixed, self.ubar, iters=iters)
        if key is not None:
            self._refs[key] = ref
        return ref


def _problem(case):
    if case not in _PROBLEMS:
        _PROBLEMS[case] = _Problem(case)
    return _PROBLEMS[case]


def solve_raw(c, F, rtol, maxit):
    """mfh_solve (one right-hand side) / mfh_solve_batch through ctypes: (status, u [nrhs, n], [info]); the status is OK or NOT_CONVERGED"""
    F = np.ascontiguousarray(np.atleast_2d(F), dtype=np.float64)
    nrhs = F.shape[0]
    u = np.full(F.shape, np.nan)
    infos = (L.SolveInfo * nrhs)()
    fn = c.lib.mfh_solve if nrhs == 1 else c.lib.mfh_solve_batch
    st = fn(c.h, nrhs, ptr(F), ptr(u), float(rtol), int(maxit), infos)
    assert st in (L.OK, L.ERR_NOT_CONVERGED), (st, c.lib.mfh_last_error(c.h).decode())
    return st, u, [i.as_dict() for i in infos]


def _set(c, opts):
    o = dict(DEFAULTS)
    o.update(opts)
    for k, v in o.items():
        c.set_option(k, v)


def _hook(c, fixed):
    def apply(r):
        z = c.debug_apply_precond(np.where(fixed, 0.0, r))[0]
        return np.where(fixed, 0.0, z)
    return apply


def _setup(case, loop):
    pre, precond, opts, batched, mkind, tau = LOOPS[loop]
    p = _problem(case)
    c = p.context(pre)
    c.set_preconditioner(precond)
    _set(c, opts)
    apply_M = p.bj if mkind == "oracle" else _hook(c, p.fixed)
    return p, c, opts, batched, mkind, apply_M, tau


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _check_iterate(p, u, info, ref, k, tau, what, converged=False, f=None, floor=False):
    """one returned vector against iterate k of the reference; returns the relative deviation of the iterate. floor: the reference residual
    of this iterate is rounding alone (the two-eigenvector right-hand side at its second iteration, 1e-15: no digit of it is determined),
    so the reported residuals are held to the bound of that right-hand side, 1e-12, instead of being compared with it"""
    assert info["converged"] == (1 if converged else 0) and info["iterations"] == k, (what, info)
    assert np.array_equal(u[p.fixed], p.ubar[p.fixed]), what + ": fixed rows"
    err = _rel(u, ref.u[k])
    assert err <= tau, "%s: iterate %.3e > %.1e" % (what, err, tau)
    if floor:
        assert ref.res[k] <= 1e-12 and info["rel_residual"] <= 1e-12 and info["true_rel_residual"] <= 1e-12, (what, info, ref.res[k])
        return err
    res, rtau = ref.res[k], tau
    if tau == TAU_FP32_ITERATE:          # another preconditioner than the reference's: the residual of the returned iterate itself
        r = np.where(p.fixed, 0.0, f - p.K @ u)
        res, rtau = float(np.sqrt(P.dot_longdouble(r, r) / ref.bb)), TAU_HOOK
    rres = abs(info["rel_residual"] / res - 1.0)
    assert rres <= 10 * rtau, "%s: rel_residual %.17g vs %.17g (%.2e)" % (what, info["rel_residual"], res, rres)
    tres = abs(info["true_rel_residual"] / res - 1.0)
    assert tres <= 1e-9, "%s: true_rel_residual %.17g vs %.17g" % (what, info["true_rel_residual"], res)
    return err


def _paths(loop, k):
    """(pcg_graph, check_every) of the runs that perform exactly k iterations"""
    paths = [(0, 50), (0, 1)] if k == 3 else [(0, 50)]
    multigrid = "mg" in loop
    if k > 1 and (not multigrid or k % 2 == 0):          # the multigrid loops shorten their blocks to 2
        paths.append((1, k))
    return paths


@pytest.mark.timeout(10)        # measured on the MI355X: 0.01 .. 0.25 s per case; 3 x that, floored at 10 s (creating a context and loading the library vary with the machine more than the solves do)
@pytest.mark.parametrize("case,loop", GRID, ids=_IDS)
def test_iterates_match_the_reference_recurrence(case, loop):
    t0 = time.perf_counter()
    p, c, opts, batched, mkind, apply_M, tau = _setup(case, loop)
    worst = 0.0
    try:
        sizes = BATCHES[p.bs] if batched else (1,)
        for nr in sizes:
            refs = [p.reference(p.F[q], apply_M, key=("bj", q) if mkind == "oracle" else None) for q in range(nr)]
            for k in KS:
                for graph, every in _paths(loop, k):
                    c.set_option("pcg_graph", graph)
                    c.set_option("check_every", every)
                    st, U, infos = solve_raw(c, p.F[:nr], 1e-30, k)
                    what = "%s %s nr=%d k=%d graph=%d" % (case, loop, nr, k, graph)
                    assert st == L.ERR_NOT_CONVERGED, what
                    assert infos[0]["used_graph"] == graph, (what, infos[0])
                    for q in range(nr):
                        assert infos[q]["reserved"] == nr, (what, infos[q])
                        worst = max(worst, _check_iterate(p, U[q], infos[q], refs[q], k, tau, what + " row %d" % q, f=p.F[q]))
    finally:
        c.close()
    print("%s %s: worst iterate deviation %.2e (bound %.0e), %.2f s" % (case, loop, worst, tau, time.perf_counter() - t0))


SINGLE = [(c, l) for c, l in GRID if not LOOPS[l][3]]


@pytest.mark.timeout(10)        # measured: 0.01 .. 0.05 s per case; floored as above
@pytest.mark.parametrize("case,loop", SINGLE, ids=["%dD-P%d-%s-%s-%s" % (c + (l,)) for c, l in SINGLE])
def test_exact_stop_and_closed_gates(case, loop):
    """rtol between the residual of k* and the smallest before it: converged at exactly k* with x_k*, eagerly with a check after every
    iteration and from a captured block of 8 whose later iterations run behind closed gates."""
    p, c, opts, batched, mkind, apply_M, tau = _setup(case, loop)
    try:
        ref = p.reference(p.F[0], apply_M, key=("bj", 0) if mkind == "oracle" else None)
        ks, rtol = P.exact_stop(ref.res)
        got = {}
        for graph, every in ((0, 1), (1, 8)):
            c.set_option("pcg_graph", graph)
            c.set_option("check_every", every)
            st, U, infos = solve_raw(c, p.F[:1], rtol, 16)
            what = "%s %s k*=%d rtol=%.3e graph=%d" % (case, loop, ks, rtol, graph)
            assert st == L.OK, what
            _check_iterate(p, U[0], infos[0], ref, ks, tau, what, converged=True, f=p.F[0])
            got[graph] = U[0]
        if loop.startswith("det"):
            assert np.array_equal(got[0], got[1]), "deterministic 1: eager and graph runs differ"
    finally:
        c.close()


def _common_rtol(histories, k_min):
    """The largest rtol (of a fine geometric grid) that every history crosses with a margin of 0.5 % on either side -- its residual at the
    crossing that far below the threshold, every earlier one that far above -- the first history at an iteration >= k_min. Rounding moves a
    residual by 1e-10 relative at the most (the bound asserted on rel_residual), seven decades inside the margin, so no row's stopping
    iteration depends on it. (The 5 % of exact_stop on either side would leave no room between the histories of eight rows.)"""
    for rtol in np.geomspace(0.5, 1e-8, 20000):
        ok = True
        for q, h in enumerate(histories):
            hit = np.nonzero(h <= rtol)[0]
            ok = ok and len(hit) > 0 and h[hit[0]] <= 0.995 * rtol and (hit[0] == 0 or 0.995 * min(h[:hit[0]]) >= rtol) and (q > 0 or hit[0] >= k_min)
        if ok:
            return float(rtol)
    raise AssertionError("no common threshold")


BATCHED = [(c, l) for c, l in GRID if LOOPS[l][3] and c[3] == "zero" and c[2] == "elasticity" and c[1] == 2]


@pytest.mark.timeout(10)        # measured: 0.1 .. 0.25 s per case, and up to 2 s more for the first case of a mesh (the two eigenvectors); floored as above
@pytest.mark.parametrize("case,loop", BATCHED, ids=["%dD-P%d-%s-%s-%s" % (c + (l,)) for c, l in BATCHED])
def test_per_vector_control_in_batches(case, loop):
    """Rows: a random vector, the same scaled by 1e3, a zero vector, the two-eigenvector right-hand side (with block-Jacobi it freezes at
    iteration 2 while its mates run on), further random vectors: 3D 6 + 2 rows, 2D 3 + 3. Each row equals its own reference iterate at
    its own stopping iteration; the zero row returns exactly 0 with iterations == 0."""
    p, c, opts, batched, mkind, apply_M, tau = _setup(case, loop)
    try:
        eig = p.eig_rhs()
        if p.dim == 3:
            F = np.stack([p.F[0], 1e3 * p.F[0], 0 * p.F[0], eig, p.F[1], p.F[2], eig, p.F[3]])
            sizes = [6] * 6 + [2] * 2
        else:
            F = np.stack([p.F[0], 1e3 * p.F[0], 0 * p.F[0], eig, p.F[1], p.F[2]])
            sizes = [3] * 6
        refs = [None if not np.any(f) else p.reference(f, apply_M, iters=100) for f in F]
        rtol = _common_rtol([r.res for r in refs if r is not None], 3)
        c.set_option("pcg_graph", 0)
        c.set_option("check_every", 1)
        runs = [(0, 1), (1, 8)]
        for graph, every in runs:
            c.set_option("pcg_graph", graph)
            c.set_option("check_every", every)
            st, U, infos = solve_raw(c, F, rtol, 104)
            assert st == L.OK
            stops = []
            for q, ref in enumerate(refs):
                what = "%s %s row %d graph=%d rtol=%.3e" % (case, loop, q, graph, rtol)
                assert infos[q]["reserved"] == sizes[q], (what, infos[q])
                if ref is None:
                    assert infos[q]["converged"] == 1 and infos[q]["iterations"] == 0 and np.all(U[q] == 0.0), what
                    continue
                ks = int(np.nonzero(ref.res <= rtol)[0][0])
                stops.append(ks)
                _check_iterate(p, U[q], infos[q], ref, ks, tau, what, converged=True, f=F[q], floor=mkind == "oracle" and F[q] is not None and np.array_equal(F[q], eig))
            assert stops[0] == stops[1] and stops[0] >= 3, stops
            if mkind == "oracle":
                assert stops[2] == 2 and len(set(stops)) > 1, stops          # the two-eigenvector row froze at 2 while its mates ran on
    finally:
        c.close()


@pytest.mark.timeout(10)
def test_both_parities_of_the_row_count_occur():
    """the pair-per-lane kernels run their single-row tail for an odd row count only"""
    rows = {case: _problem(case).n_dof for case in CASES}
    assert {n % 2 for n in rows.values()} == {0, 1}, rows
    assert rows[(3, 2, "elasticity", "zero")] == 1509, rows


# ------------------------------------------------------------------------------------------------ past the grid caps
def _big_problem(dim, size):
    """A P1 context on the assembled SpMV (both triangles), K = its own export (pinned at scale by test_gpu_parity_at_scale.py), the face
    x = min fixed at zero."""
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(*size) if dim == 3 else grid.grid_tri_mesh(*size)
    V, T = np.asarray(V, dtype=np.float64), np.asarray(T)
    c = M.Context(0)
    c.set_option("matrix_free", 0)
    c.set_option("matrix_storage", 0)
    c.mesh_build(T, V, 1)
    c.material_isotropic(200.0, 0.35)
    c.assemble()
    K = c.export_scipy()
    nodes = np.nonzero(V[:, 0] < V[:, 0].min() + 1e-9)[0]
    var = (nodes[:, None] * dim + np.arange(dim)).ravel()
    c.fix_variables(var, np.zeros(len(var)))
    fixed = np.zeros(K.shape[0], bool)
    fixed[var] = True
    return c, K, fixed


def _past_cap(c, K, fixed, dim, nr, opts, min_rows):
    """k = 3 against the FP64 reference on scipy; the bound is the reference's own: 100 x |x_3(FP64 dots) - x_3(longdouble dots)|,
    floored at 1e-13 and asserted to stay <= 1e-10"""
    n_rows = K.shape[0] // dim
    assert n_rows > min_rows, n_rows
    F = np.random.default_rng(51).standard_normal((nr, K.shape[0]))
    apply_K, bj = P.csr_apply(K), P.block_jacobi_apply(K, dim, fixed)
    c.set_preconditioner(BJ)
    _set(c, opts)
    c.set_option("pcg_graph", 0)
    st, U, infos = solve_raw(c, F, 1e-30, 3)
    assert st == L.ERR_NOT_CONVERGED
    for q in range(nr):
        ref = P.pcg_classic(apply_K, bj, F[q], fixed, iters=3)
        ref64 = P.pcg_classic(apply_K, bj, F[q], fixed, iters=3, dot=P.dot_fp64)
        tau = max(100 * _rel(ref64.u[3], ref.u[3]), 1e-13)
        assert tau <= 1e-10, tau
        err = _rel(U[q], ref.u[3])
        print("rows %d nr %d row %d: deviation %.2e, bound %.2e" % (n_rows, nr, q, err, tau))
        assert infos[q]["iterations"] == 3 and infos[q]["converged"] == 0
        assert np.all(U[q][fixed] == 0.0)
        assert err <= tau, (err, tau)
        assert abs(infos[q]["rel_residual"] / ref.res[3] - 1.0) <= 10 * tau
        assert abs(infos[q]["true_rel_residual"] / ref.res[3] - 1.0) <= 1e-9


@pytest.mark.timeout(10)        # measured: 1.4 s; 3 x, floored as above
def test_past_the_cap_of_the_two_rows_per_lane_kernels():
    """More than 2048 x 256 x 2 = 1 048 576 rows: k_pcg_update and k_cg_update1 run their grid-stride loops (2D P1, 730 x 724 quads:
    1 058 495 rows, odd)."""
    c, K, fixed = _big_problem(2, (730, 724))
    try:
        for opts in (dict(pcg_variant=0), dict(pcg_variant=1)):
            _past_cap(c, K, fixed, 2, 1, opts, 1048576)
    finally:
        c.close()


@pytest.mark.timeout(10)        # measured: 0.25 s and 0.49 s; floored as above
@pytest.mark.parametrize("dim,size,nr,min_rows", [(2, (300, 292), 3, 174848), (3, (26, 26, 26), 6, 87424)])
def test_past_the_cap_of_the_lane_per_row_and_vector_kernels(dim, size, nr, min_rows):
    """More than 3 x 683 x 256 = 524 544 (row, vector) pairs: k_cg_init and k_cg_update stride, a lane keeps its vector."""
    c, K, fixed = _big_problem(dim, size)
    try:
        _past_cap(c, K, fixed, dim, nr, dict(pcg_variant=1, batch_rhs=1), min_rows)
    finally:
        c.close()


@pytest.mark.timeout(10)        # measured: 0.21 s; floored as above
def test_direction_kernel_under_vec_grid_cap():
    """vec_grid_cap 256 (the option's minimum) on the 3D P2 mesh. Its 4 527 doubles fill 9 workgroups of k_pcg_direction, so this pins the
    option's plumbing and the odd tail; the stride loop itself needs more than 256 x 256 pairs and runs on the 26^3 P1 mesh
    (138 022 pairs, 540 workgroups uncapped) with the reference's own bound of the past-cap tests."""
    p = _problem((3, 2, "elasticity", "zero"))
    ref = p.reference(p.F[0], p.bj, key=("bj", 0))
    c = p.context()
    try:
        c.set_preconditioner(BJ)
        _set(c, dict(pcg_variant=0, pcg_graph=0))
        c.set_option("vec_grid_cap", 256)
        st, U, infos = solve_raw(c, p.F[:1], 1e-30, 3)
        assert st == L.ERR_NOT_CONVERGED
        _check_iterate(p, U[0], infos[0], ref, 3, TAU_ORACLE, "vec_grid_cap 256")
    finally:
        c.set_option("vec_grid_cap", 16384)          # the option is process-global
        c.close()
    c, K, fixed = _big_problem(3, (26, 26, 26))
    try:
        c.set_option("vec_grid_cap", 256)
        _past_cap(c, K, fixed, 3, 1, dict(pcg_variant=0), 87424)
    finally:
        c.set_option("vec_grid_cap", 16384)
        c.close()
