"""The two loops on the pencil A = cK K + cM M -- the PCG of mfh_newmark (NewmarkWork::solve: k_dyn_init / update / rz / direction) and the COCG of
mfh_harmonic (HarmonicWork::solve: k_harm_init / update / rz / direction, the complex alpha and beta formed on the device) -- ITERATE BY ITERATE
against the reference recurrences of tests/pencil_iterates_util.py, and their shared block-Jacobi blocks (k_pencil_dinv) as a fixed map. The loops
are reached through the hooks mfh_debug_newmark_pcg / mfh_debug_harmonic_cocg / mfh_debug_pencil_precond, which run the loops' own member
functions: with rtol = 1e-30 and maxit = k they return x_k and the scalar histories. A converged solution forgives a wrong beta, a conjugated dot
product, a dropped term of r^T z, an x that moves after the stop or a preconditioner that is merely some other SPD block-diagonal map -- the solve
only gets slower (and mfh_harmonic continues from the true residual); an iterate does not.

  a  k_pencil_dinv       z = Dinv r against the dense inverse of the d x d diagonal blocks of the oracle's cK K + cM M for (cK, cM) in
                         {(1, 4 rho / dt^2), (0, rho), (1, w^2 rho) at two frequencies, (1, 0)}; clamped, free, and with ONE component of the
                         face nodes fixed (rows and columns eliminated inside a block); |z - z_ref| <= 1e-13 |z_ref| per block (the bar of
                         tests/test_gpu_preconditioner_maps.py), z == r bit for bit on the fixed rows
  b  Newmark PCG         x_k, r.z, p.Ap, r.r at k in {1, 2, 3, 5, 8}: the time-step pencil and the initial-acceleration pencil (cK = 0), from
                         zero and from a non-zero start; block-Jacobi (oracle blocks), two-level and multigrid (apply_M = debug_apply_precond)
                         on every mesh -- under a hierarchy at k in {1, 2, 3}, and to k = 8 where the reference floor holds (HOOK_PCG_FULL)
  c  COCG                the same for every damping case of harmonic_util at its five frequencies, real and complex load, one warm start;
                         r^T z and p^T Z p as complex numbers; block-Jacobi of K + w^2 rho M; multigrid (the hook on each plane) and two-level
                         on (3, 2): every input at k in {1, 2, 3}, the two lowest frequencies to k = 8 (_cocg_ks: the floor is held per k)
  d  the stop            rtol between the residuals of k* - 1 and k* (pcg_iterates_util.exact_stop): its == k* and x == x_k* with check_every 2 and
                         with check_every 50 (the batch runs past k* behind closed gates: nothing of the later iterations is written), bit-identical
                         under deterministic 1
  e  dyn_grid_cap 1      one workgroup per vector kernel on the 510 block rows of (3, 2): the lanes loop
  f  harmonic_two_pass 1 the two-launch form of the mass product inside the loop

Bounds, from the reference alone (pencil_iterates_util): tau_k = max(floor, 100 x the gap between the reference's FP64 and extended-precision walks
at k), floor = 1e-12 where apply_M comes from the oracle and 1e-11 where it is the hook; the scalars in the scales |r||z|, |p||Z p| (2-norms, of the
complex vectors for the COCG: a dot product rounds in proportion to sum |r_i||z_i|, and r^T z itself may cancel) and r.r relative. Where apply_M is
the hook the gap is measured here, with the hook in both walks, and held to the same 1e-11 as the CPU test holds the block-Jacobi inputs: no input
is skipped. The unfused mg_precond call of the two loops (no MgFuse) smooths with the FP64 inverse blocks -- the FP32 copy is read by the fused
kernels of mfh_solver.cpp alone -- so the hook's map is the loop's map under the default mg_dinv_fp32 1 and no mg_* option is changed here; the
PCG walks of the two hierarchies run under deterministic 1 (HOOK_PCG_FULL says why).
Both hierarchies build on every small mesh; every case asserts that the loops ran the preconditioner it names (info["precondUsed"]).

Measured on the MI355X (first run; worst error / tau): see docs/design/04_5_pcg_vector_kernels.md, "Iterates pinned"."""
import functools
import time

import numpy as np
import pytest

import meshfem_amd as M

import dynamics_util as D
import harmonic_util as H
import modes_util as U
import pcg_iterates_util as P
import pencil_iterates_util as R

pytestmark = pytest.mark.gpu

PRECONDS = {"jacobi": M.PRECOND_BLOCK_JACOBI, "two-level": M.PRECOND_TWO_LEVEL, "multigrid": M.PRECOND_MULTIGRID}
KS = R.KS


def _name(v):
    return "%dD-P%d" % v if isinstance(v, tuple) else str(v)


def _context(key, precond="jacobi", options=(), fixed="clamp"):
    V, T, deg, _ = U.mesh_arrays(key)
    c = M.Context(0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    c.set_preconditioner(PRECONDS[precond])
    fv = _fixed_vars(key, fixed)
    if len(fv):
        c.fix_variables(fv)
    assert np.array_equal(c.node_positions(), U.fem_mesh(key).node_pos)          # the oracle's node numbering is the library's own
    return c


def _fixed_vars(key, fixed):
    """"clamp": every variable of the nodes on the face x = min; "component": their y components alone; "free": none"""
    v = U.clamp_vars(key)
    d = U.fem_mesh(key).N
    return {"clamp": v, "component": v[v % d == 1], "free": v[:0]}[fixed]


def _apply_M(c, key, floor_precond):
    """(apply_M of the reference, floor of tau, what ran): the oracle's block-Jacobi for a block-Jacobi context, else the device hook. Both
    hierarchies build on every small mesh (clamped): a loop that fell back to block-Jacobi is a failure here, not a second Jacobi case."""
    info = c.newmark(1.0, 0, a0=np.zeros(c.bs * c.n_dof))["info"]          # no step, no solve: the choice mfh_newmark and mfh_harmonic make
    used = info["precondUsed"]
    assert used == PRECONDS[floor_precond], "%s asked for %s, the loops run %d (%s)" % (_name(key), floor_precond, used, info["note"])
    if used == M.PRECOND_BLOCK_JACOBI:
        return None, R.TAU_ORACLE, used
    return R.hook_apply(key, lambda r: c.debug_apply_precond(r)[0]), R.TAU_HOOK, used


class _Worst:
    def __init__(self):
        self.x = self.s = self.gap = 0.0

    def iterate(self, what, x, x0, ref, k, free, fixed):
        assert np.array_equal(x[fixed], x0[fixed]), what + ": fixed rows"
        err = R.rel(x[free], ref.x[k])
        self.x = max(self.x, err / ref.tau_x[k])
        assert err <= ref.tau_x[k], "%s: iterate %d off by %.3e > %.1e" % (what, k, err, ref.tau_x[k])

    def scalar(self, what, got, want, scale, tau):
        err = abs(got - want) / scale
        self.s = max(self.s, err / tau)
        assert err <= tau, "%s: %.17g vs %.17g, %.3e of the scale > %.1e" % (what, got, want, err, tau)

    def floor(self, what, ref, hook, upto=None):
        gx, gs = ref.gap_x[:upto], ref.gap_s[:upto]
        self.gap = max(self.gap, gx.max(), gs.max())
        if hook:          # (the block-Jacobi inputs are held to the floor by tests/test_pencil_iterates_reference.py)
            assert gx.max() <= R.FLOOR_MAX and gs.max() <= R.FLOOR_MAX, "%s: the reference's own floor %.2e / %.2e: replace this input" % (what, gx.max(), gs.max())


def _check_real_history(w, what, hist, ref, k):
    for j in range(k + 1):
        w.scalar("%s r.z[%d]" % (what, j), hist[j, 0], ref.rz[j], ref.rz_scale[j], ref.tau_s[j])
        w.scalar("%s r.r[%d]" % (what, j), hist[j, 2], ref.rr[j], ref.rr[j], ref.tau_s[j])
        if j < k:
            w.scalar("%s p.Ap[%d]" % (what, j), hist[j, 1], ref.pAp[j], ref.pAp_scale[j], ref.tau_s[j])


def _check_complex_history(w, what, hist, chist, ref, k):
    for j in range(k + 1):
        w.scalar("%s r^T z[%d]" % (what, j), chist[j, 0], ref.rz[j], ref.rz_scale[j], ref.tau_s[j])
        w.scalar("%s r.r[%d]" % (what, j), hist[j, 2], ref.rr[j], ref.rr[j], ref.tau_s[j])
        if j < k:
            w.scalar("%s p^T Z p[%d]" % (what, j), chist[j, 1], ref.pZp[j], ref.pZp_scale[j], ref.tau_s[j])


def _masks(key):
    _, _, free, n = R.free_pencil(key)
    fixed = np.ones(n, bool)
    fixed[free] = False
    return free, fixed


# ------------------------------------------------------------------------------------------------ a. k_pencil_dinv as a map
@pytest.mark.parametrize("fixed", ["clamp", "free", "component"])
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_pencil_dinv_is_the_inverse_of_the_diagonal_blocks(key, fixed):
    K, Mm = U.pencil(key)
    d = U.fem_mesh(key).N
    n = K.shape[0]
    fv = _fixed_vars(key, fixed)
    mask = np.zeros(n, bool)
    mask[fv] = True
    om = H.sweep_omegas(key)
    pencils = [R.newmark_pencils(key)["step"], R.newmark_pencils(key)["accel"], (1.0, om[1] ** 2 * H.DENSITY), (1.0, om[3] ** 2 * H.DENSITY), (1.0, 0.0)]
    r = np.random.default_rng(8).standard_normal(n)          # (non-zero on the fixed rows: the identity there is part of the map)
    c = _context(key, "jacobi", fixed=fixed)
    worst = 0.0
    try:
        for cK, cM in pencils:
            B = P.block_jacobi_blocks(cK * K + cM * Mm, d, mask)
            zref = np.linalg.solve(B, r.reshape(-1, d)[:, :, None])[:, :, 0]
            z = c.debug_pencil_precond(cK, cM, r)
            assert np.array_equal(z[mask], r[mask]), "cK %g cM %g: the fixed rows are not the identity" % (cK, cM)
            err = np.linalg.norm(z.reshape(-1, d) - zref, axis=1) / np.linalg.norm(zref, axis=1)
            worst = max(worst, err.max())
            assert err.max() <= 1e-13, "cK %g cM %g: block %d off by %.3e" % (cK, cM, err.argmax(), err.max())
    finally:
        c.close()
    print("%s %s: worst block error %.2e (bar 1e-13), %d of %d variables fixed" % (_name(key), fixed, worst, mask.sum(), n))
    assert fixed != "component" or (0 < mask.sum() and np.all(mask.reshape(-1, d).sum(axis=1) <= 1))


# ------------------------------------------------------------------------------------------------ b. the Newmark PCG
@functools.lru_cache(maxsize=None)
def _pcg_jacobi_reference(key, pencil, warm, iters=R.KMAX):
    b, x0 = R.newmark_rhs(key)
    cK, cM = R.newmark_pencils(key)[pencil]
    return R.pcg_reference(key, cK, cM, b, x0 if warm else None, iters=iters)


def _pcg_reference(c, key, precond, pencil, warm, iters=R.KMAX):
    apply_M, floor, used = (None, R.TAU_ORACLE, M.PRECOND_BLOCK_JACOBI) if pencil == "accel" else _apply_M(c, key, precond)
    if apply_M is None:
        return _pcg_jacobi_reference(key, pencil, warm, iters), False, used
    b, x0 = R.newmark_rhs(key)
    cK, cM = R.newmark_pencils(key)[pencil]
    return R.pcg_reference(key, cK, cM, b, x0 if warm else None, apply_M, iters, floor), True, used


# The walks under the hook preconditioners. B ~ K^-1 leaves the mass-dominated low modes of A = K + 4 rho / dt^2 M as outlying eigenvalues of B A; their
# Ritz values converge within a few iterations, and from there on ANY two FP64 walks part exponentially (Paige, Greenbaum), the faster the fewer
# unknowns there are. The reference's own floor at k = 8, measured here with the hook in both walks, from a cold start, on (2, 1), (2, 2), (3, 1), (3, 2):
#     two-level   1.8e-9    2.4e-11   4.4e-13   4.6e-14            multigrid   1.3e-7    1.5e-7    1.2e-12   2.8e-10
# and from the warm start the same or worse, while at k <= 3 it is <= 3e-14 on every mesh (the CPU stand-in of tests/test_pencil_iterates_reference.py,
# splu of K_ff as B, shows the same: <= 2e-14 at k <= 3, 7e-6 at k = 8 on (2, 1)). tau_k is per k, and so is the floor: every mesh and both starts are
# walked under both hierarchies at k in HOOK_KS = {1, 2, 3}, which pins alpha, beta, r.z from k_dyn_rz and the history columns, and to k = 8 where
# the floor holds there (HOOK_PCG_FULL). The floor is asserted up to the largest k of a walk. The hierarchies' own sums differ by 1e-14 from run to
# run, which is amplified alike -- the k = 8 floor of (3, 1) multigrid measured 1.2e-12 in two runs and 1.3e-11 in a third --, so these walks run
# under option deterministic 1, where the hook is the same map bit for bit ((3, 1) multigrid: 2.7e-12 cold, 5.6e-12 warm in every run).
HOOK_PCG_FULL = {("two-level", (3, 1)), ("two-level", (3, 2)), ("multigrid", (3, 1))}


def _pcg_options(precond):
    return (("deterministic", 1),) if precond != "jacobi" else ()


def _pcg_ks(key, precond, pencil):
    return KS if precond == "jacobi" or pencil == "accel" or (precond, key) in HOOK_PCG_FULL else R.HOOK_KS


def _run_pcg_iterates(c, key, precond, pencil):
    free, fixed = _masks(key)
    b, x0 = R.newmark_rhs(key)
    cK, cM = R.newmark_pencils(key)[pencil]
    w = _Worst()
    ks = _pcg_ks(key, precond, pencil)
    for warm in (False, True):
        ref, hook, used = _pcg_reference(c, key, precond, pencil, warm)
        start = x0 if warm else np.zeros_like(x0)
        what = "%s %s %s %s" % (_name(key), precond, pencil, "warm" if warm else "cold")
        w.floor(what, ref, hook, max(ks) + 1)
        for k in ks:
            x, hist, its = c.debug_newmark_pcg(cK, cM, b, start if warm else None, 1e-30, k)
            assert its == -1 and hist.shape == (k + 1, 4), (what, k, its)
            w.iterate(what, x, start, ref, k, free, fixed)
            _check_real_history(w, "%s k=%d" % (what, k), hist, ref, k)
    return w, used


NEWMARK = [(k, "jacobi", "accel") for k in U.SMALL] + [(k, p, "step") for k in U.SMALL for p in PRECONDS]


@pytest.mark.parametrize("key,precond,pencil", NEWMARK, ids=_name)
def test_newmark_pcg_iterates(key, precond, pencil):
    t0 = time.perf_counter()
    c = _context(key, precond, _pcg_options(precond))
    try:
        w, used = _run_pcg_iterates(c, key, precond, pencil)
    finally:
        c.close()
    print("newmark pcg %s %s %s (ran %d): worst iterate error / tau %.3e, scalars %.3e, reference floor %.2e, %.2f s" %
          (_name(key), precond, pencil, used, w.x, w.s, w.gap, time.perf_counter() - t0))
    assert used == (M.PRECOND_BLOCK_JACOBI if pencil == "accel" else PRECONDS[precond])


# ------------------------------------------------------------------------------------------------ c. the COCG
@functools.lru_cache(maxsize=None)
def _cocg_jacobi_reference(key, case, iw, kind, warm, iters=R.KMAX):
    zK, zM, cMj = R.harmonic_inputs(key, case, H.sweep_omegas(key)[iw])
    return R.cocg_reference(key, zK, zM, cMj, H.load(key, kind), _warm_start(key, case) if warm else None, iters=iters)


def _warm_start(key, case):
    """the solution of the second test frequency (zero on the clamp): what a warm-started sweep hands the third"""
    return H.reference(key, case, "complex")[1]


def _cocg_reference(c, key, precond, case, iw, kind, warm, iters=R.KMAX):
    apply_M, floor, used = _apply_M(c, key, precond)
    if apply_M is None:
        return _cocg_jacobi_reference(key, case, iw, kind, warm, iters), False, used
    zK, zM, cMj = R.harmonic_inputs(key, case, H.sweep_omegas(key)[iw])
    return R.cocg_reference(key, zK, zM, cMj, H.load(key, kind), _warm_start(key, case) if warm else None, apply_M, iters, floor), True, used


def _run_cocg_iterates(c, key, precond, case, inputs):
    """inputs: (frequency index, load kind, warm start) triples"""
    free, fixed = _masks(key)
    w = _Worst()
    used = None
    for iw, kind, warm in inputs:
        om = H.sweep_omegas(key)[iw]
        zK, zM, cMj = R.harmonic_inputs(key, case, om)
        f = H.load(key, kind)
        ref, hook, used = _cocg_reference(c, key, precond, case, iw, kind, warm)
        start = _warm_start(key, case) if warm else np.zeros(len(f), dtype=np.complex128)
        what = "%s %s %s omega[%d] %s %s" % (_name(key), precond, case, iw, kind, "warm" if warm else "cold")
        ks = _cocg_ks(precond, iw, warm)
        w.floor(what, ref, hook, max(ks) + 1)
        for k in ks:
            x, hist, chist, its = c.debug_harmonic_cocg(zK, zM, cMj, f, start if warm else None, 1e-30, k)
            assert its == -1 and hist.shape == (k + 1, 4) and chist.shape == (k + 1, 2), (what, k, its)
            w.iterate(what, x, start, ref, k, free, fixed)
            _check_complex_history(w, "%s k=%d" % (what, k), hist, chist, ref, k)
            if case == "undamped" and kind == "real" and not warm:
                assert np.all(x.imag == 0.0) and np.all(chist.imag == 0.0), what + ": a real system stays real"
    return w, used


ALL_INPUTS = [(iw, kind, False) for iw in range(H.N_FREQ) for kind in R.KINDS] + [(2, "complex", True)]
# The walks under the hook preconditioners: above the first resonances Z is indefinite, B ~ K^-1 is no preconditioner of it, and the reference's own
# floor at k = 8 (the hook in both walks) reaches 1e-11 ... 1e-8 from mid(omega_2, omega_3) on, on every mesh and for both hierarchies (two-level on
# (3, 2), undamped, mid(omega_5, omega_6): 1e-12 in one run, 1.1e-11 in the next), and from the warm start. At 0 and omega_1 / 2 it measured <= 5e-13 in
# every run. The floor is per k, as tau_k is: every frequency, both loads and the warm start are walked at k in HOOK_KS = {1, 2, 3} (k_harm_rz and the
# complex alpha and beta on an indefinite Z; measured floor over these walks <= 3.5e-13), the two lowest frequencies to k = 8.
def _cocg_ks(precond, iw, warm):
    return KS if precond == "jacobi" or (iw in (0, 1) and not warm) else R.HOOK_KS


HARMONIC = [(k, p) for k in U.SMALL for p in ("jacobi", "multigrid")] + [((3, 2), "two-level")]


@pytest.mark.parametrize("case", list(H.CASES))
@pytest.mark.parametrize("key,precond", HARMONIC, ids=_name)
def test_harmonic_cocg_iterates(key, precond, case):
    t0 = time.perf_counter()
    c = _context(key, precond)
    try:
        w, used = _run_cocg_iterates(c, key, precond, case, ALL_INPUTS)
    finally:
        c.close()
    print("harmonic cocg %s %s %s (ran %d): worst iterate error / tau %.3e, scalars %.3e, reference floor %.2e, %.2f s" %
          (_name(key), precond, case, used, w.x, w.s, w.gap, time.perf_counter() - t0))
    assert used == PRECONDS[precond]


# ------------------------------------------------------------------------------------------------ d. the stop
STOP_MAXIT = 40


def _stop_runs(key, precond, run, reference):
    """run(c, rtol) -> (x, hist, its); reference(c) -> (ref, hook). its == k* and x == x_k* with check_every 2 and 50, without and with
    deterministic 1 (there bit for bit); nothing of an iteration >= k* is written but its r.z and r.r"""
    free, fixed = _masks(key)
    w = _Worst()
    for det in (0, 1):
        c = _context(key, precond, (("deterministic", det),))
        try:
            ref, hook = reference(c)
            ks, rtol = R.stop_rule(ref.res)
            what = "%s %s deterministic %d k*=%d rtol=%.3e" % (_name(key), precond, det, ks, rtol)
            w.floor(what, ref, hook, ks + 1)
            got = {}
            for every in (2, 50):
                c.set_option("check_every", every)
                x, hist, its = run(c, rtol)
                assert its == ks, "%s check_every %d: stopped at %d" % (what, every, its)
                w.iterate("%s check_every %d" % (what, every), x, np.zeros_like(x), ref, ks, free, fixed)
                w.scalar(what + " r.r at the stop", hist[ks, 2], ref.rr[ks], ref.rr[ks], ref.tau_s[ks])
                assert hist[ks, 2] <= rtol * rtol * ref.bb < hist[:ks, 2].min(), what
                assert np.all(hist[ks + 1:] == 0.0) and hist[ks, 1] == 0.0, "%s check_every %d: an iteration behind the closed gate wrote its sums" % (what, every)
                got[every] = x
            if det:
                assert np.array_equal(got[2], got[50]), what + ": the two batch lengths differ"
        finally:
            c.close()
    return w, ks


@pytest.mark.parametrize("precond", ["jacobi", "multigrid"])
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_newmark_pcg_stops_at_the_first_iterate_below_the_threshold(key, precond):
    b, _ = R.newmark_rhs(key)
    cK, cM = R.newmark_pencils(key)["step"]
    w, ks = _stop_runs(key, precond, lambda c, rtol: c.debug_newmark_pcg(cK, cM, b, None, rtol, STOP_MAXIT),
                       lambda c: _pcg_reference(c, key, precond, "step", False, R.STOP_ITERS)[:2])
    print("newmark stop %s %s: k* = %d, worst iterate error / tau %.3e" % (_name(key), precond, ks, w.x))


@pytest.mark.parametrize("precond", ["jacobi", "multigrid"])
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_harmonic_cocg_stops_at_the_first_iterate_below_the_threshold(key, precond):
    case, om = R.stop_harmonic(key)
    iw = int(np.nonzero(H.sweep_omegas(key) == om)[0][0])
    zK, zM, cMj = R.harmonic_inputs(key, case, om)
    f = H.load(key, "complex")

    def run(c, rtol):
        x, hist, chist, its = c.debug_harmonic_cocg(zK, zM, cMj, f, None, rtol, STOP_MAXIT)
        if its >= 0:
            assert np.all(chist[its + 1:] == 0.0) and chist[its, 1] == 0.0          # the complex history behind the closed gate
        return x, hist, its
    w, ks = _stop_runs(key, precond, run, lambda c: _cocg_reference(c, key, precond, case, iw, "complex", False, R.STOP_ITERS)[:2])
    print("harmonic stop %s %s: k* = %d, worst iterate error / tau %.3e" % (_name(key), precond, ks, w.x))


# ------------------------------------------------------------------------------------------------ e, f. past the grid cap, and in two passes
@pytest.mark.parametrize("precond", ["jacobi", "two-level"])
def test_newmark_pcg_with_one_workgroup(precond):
    """dyn_grid_cap 1 on (3, 2): 551 block rows (510 of them free) in one workgroup of 256 lanes, 1 653 variables in one workgroup of k_dyn_rz /
    k_dyn_direction"""
    key = (3, 2)
    assert U.pencil(key)[0].shape[0] // 3 == 551 and len(R.free_pencil(key)[2]) // 3 == 510
    c = _context(key, precond, (("dyn_grid_cap", 1),))
    try:
        w, used = _run_pcg_iterates(c, key, precond, "step")
    finally:
        c.close()
    print("newmark pcg one workgroup %s: worst iterate error / tau %.3e, scalars %.3e" % (precond, w.x, w.s))
    assert used == PRECONDS[precond]


@pytest.mark.parametrize("options", [(("dyn_grid_cap", 1),), (("harmonic_two_pass", 1),)], ids=["cap-1", "two-pass"])
@pytest.mark.parametrize("precond", ["jacobi", "multigrid"])
def test_harmonic_cocg_with_one_workgroup_and_in_two_passes(precond, options):
    key = (3, 2)
    c = _context(key, precond, options)
    try:
        inputs = [(2, "complex", False), (0, "real", False), (2, "complex", True)]
        w, used = _run_cocg_iterates(c, key, precond, "rayleigh", inputs)
    finally:
        c.close()
    print("harmonic cocg %s %s: worst iterate error / tau %.3e, scalars %.3e" % (options, precond, w.x, w.s))
    assert used == PRECONDS[precond]


# ------------------------------------------------------------------------------------------------ after a solve
@pytest.mark.parametrize("key,precond", [((3, 1), "jacobi"), ((3, 1), "multigrid"), ((3, 2), "jacobi"), ((3, 2), "two-level")], ids=_name)
def test_loops_after_a_solve(key, precond):
    """mfh_solve leaves K assembled on the upper-triangle pattern (the automatic storage of the matrix-free operator); the loops need both triangles
    and switch the pattern for their call. The switch has to come before the preconditioner is chosen and k_pencil_dinv reads K: made inside
    ensure_mass, after ensure_precond had returned early on the assembled K, it dropped the hierarchy just chosen (block-Jacobi ran in its place)
    and left K's values of the upper pattern under the wide one (r.z of iteration 0 off by 16 x). Same walks, same bounds, and mfh_newmark itself
    reports the context's preconditioner as on a fresh context."""
    b, _ = R.newmark_rhs(key)
    i = D.case_inputs(key, "undamped")
    fresh = _context(key, precond, _pcg_options(precond))
    want = fresh.newmark(i["dt"], 3, f=b, density=D.DENSITY, rtol=1e-10)["info"]
    fresh.close()
    c = _context(key, precond, _pcg_options(precond))
    try:
        c.solve(b, rtol=1e-6)
        got = c.newmark(i["dt"], 3, f=b, density=D.DENSITY, rtol=1e-10)["info"]
        assert got["precondUsed"] == want["precondUsed"] == PRECONDS[precond]
        assert abs(got["iterationsTotal"] - want["iterationsTotal"]) <= 0.05 * want["iterationsTotal"], (got, want)          # (the V-cycle's sums are not ordered: a step may take one more)
        c.solve(b, rtol=1e-6)
        w1, _ = _run_pcg_iterates(c, key, precond, "step")
        c.solve(b, rtol=1e-6)
        w2, _ = _run_cocg_iterates(c, key, precond, "rayleigh", [(1, "complex", False)])
    finally:
        c.close()
    print("after a solve %s %s: worst iterate error / tau %.3e (pcg), %.3e (cocg)" % (_name(key), precond, w1.x, w2.x))
