"""The block LOBPCG loop of mfh_modes / mfh_modes_many / mfh_buckling / mfh_modes_prestressed (lobpcg_run over struct Lobpcg,
meshfem_amd/csrc/mfh_modes.hip) ITERATE BY ITERATE against the reference recurrence of tests/lobpcg_iterates_util.py, on all three pencils. The loop
is reached through the hook mfh_debug_lobpcg, which goes through modes_prepare and lobpcg_run themselves from a start block of the caller's: with
rtol = 1e-30 and maxit = k it hands out the whole block X_k and, per convergence check, the m Ritz values, the m relative residuals and
{|W|, |P|, restarts}. A converged eigenpair forgives a P block that keeps its X rows, a P block that is dropped every iteration, a W that is not
projected against the rigid modes or the deflation set, a soft lock on the wrong columns, images combined with the wrong coefficient block, a
density missing from one image family, a stale haveP -- the loop only needs more iterations; an iterate forgives none of it.

  a  vibration, clamped     (K, rho M) on the four small meshes, nev 1 and 4 (m = 3, 6), S0 seeded normal values (non-zero on the fixed rows),
                            k in {1, 2, 3, 5, 8} under block-Jacobi (oracle blocks); two-level and multigrid (T = debug_apply_precond, option
                            deterministic 1) at k in {1, 2, 3}; density 2.7 once
  b  vibration, free body   (2, 2) and (3, 1): Z from modes_util.rigid_modes; |Z^T M X_k| <= tau besides
  c  the full block         nev 20 on (3, 2): m = 24, a 72 x 72 basis, k in {1, 2, 3}
  d  buckling               (Kg, K) on col3d-P1 and strip-P2, nev 3, the inner product K's: under axial compression (Kg negative semidefinite, every
                            mu negative) and under a random symmetric prestress field (Ritz values of both signs in the start block)
  e  prestressed            (K + s Kg, rho M) on the same at 0.5 and 1.1 x the critical factor (A indefinite at 1.1)
  f  deflation              a set of 7 M-orthonormal random columns on (3, 1) and (2, 2); |(M Q)^T X_k| <= tau besides
  g  the stop and the lock  rtol from the reference's own residual histories (lobpcg_iterates_util.find_stop: every residual a factor 2 away):
                            iterations == k*, |W| and |P| per iteration, X at the stop, the same bits twice under deterministic 1
  h  the space runs out     two triangles, nEff = 4 = m: iterations == 0 and lam == eigh; nEff = 5, m = 4: all but one column of W dropped, and
                            after one iteration lam == eigh whichever columns went
  i  the public entry point modes_prestressed(x0=..., maxit=k) runs k iterations and returns finite numbers

What is compared, and the bounds tau_k = max(floor, 100 x the reference's FP64-vs-extended gap at k): see lobpcg_iterates_util. floor = 1e-12 where
T comes from the oracle's blocks, 1e-11 where it is the device hook; there the gap is measured here, with the hook in both walks, and held to
FLOOR_MAX like the CPU test holds the others. Also, on the device history alone: no Ritz value rises from one check to the next by more than tau
(Cauchy interlacing), and the fixed variables stay +-0.0 in every column.
Measured on the MI355X (first run; worst error / tau): docs/design/04_12_modes.md, "Iterates pinned"."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import meshfem_amd as M
from meshfem_amd import _lib
from oracle import meshfem_oracle as O

import buckling_util as B
import lobpcg_iterates_util as LU
import modes_util as U
import prestress_util as PS

pytestmark = pytest.mark.gpu

PRECONDS = {"jacobi": M.PRECOND_BLOCK_JACOBI, "two-level": M.PRECOND_TWO_LEVEL, "multigrid": M.PRECOND_MULTIGRID}
HOOK_OPTIONS = (("deterministic", 1), ("matrix_storage", 0))          # the hook and the loop then see one pattern and one map, bit for bit


def _context(case, precond="jacobi", options=()):
    V, T, deg, _ = B.mesh_arrays(case.key)
    c = M.Context(0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    c.set_preconditioner(PRECONDS[precond])
    if not case.free:
        c.fix_variables(B.clamp_vars(case.key))
    if case.pencil != "vibration":
        c.set_prestress(LU.prestress(case))
    assert np.array_equal(c.node_positions(), B.fem_mesh(case.key).node_pos)          # the oracle's node numbering is the library's own
    return c


def _load_factor(case):
    return case.ratio * PS.critical_factor(case.key) if case.pencil == "prestressed" else 0.0


def _run(c, case, p, maxit, rtol=1e-30):
    Q = None if p.Q is None else LU.expand(p, p.Q)
    out = c.debug_lobpcg(case.pencil, p.S0, case.nev, density=case.density, load_factor=_load_factor(case), free_body=case.free, rtol=rtol,
                         maxit=maxit, Q=Q)
    assert out["m"] == p.m == c.debug_lobpcg_block_size(case.pencil, case.nev, case.free, case.nq)
    return out


class _Worst:
    def __init__(self):
        self.lam = self.res = self.sub = self.extra = 0.0

    def __str__(self):
        return "worst error / tau: lam %.3f res %.3f subspace %.3f other %.3f" % (self.lam, self.res, self.sub, self.extra)


def _check_history(w, what, p, ref, out, calls):
    """Ritz values, residuals and sets of the first `calls` convergence checks; monotone Ritz values on the device history alone"""
    for k in range(calls):
        e_lam, e_res, _ = LU.measures(p, ref, k, out["lam"][k], out["res"][k], None)
        w.lam, w.res = max(w.lam, e_lam / ref.tau_lam[k]), max(w.res, e_res / ref.tau_res[k])
        assert e_lam <= ref.tau_lam[k], "%s: Ritz values at k = %d off by %.3e > %.1e" % (what, k, e_lam, ref.tau_lam[k])
        assert e_res <= ref.tau_res[k], "%s: residuals at k = %d off by %.3e > %.1e" % (what, k, e_res, ref.tau_res[k])
        assert tuple(out["sets"][k]) == tuple(ref.sets[k]), "%s: |W|, |P|, restarts at k = %d: %s, the reference has %s" % (what, k, out["sets"][k], ref.sets[k])
    rise = LU.monotone_defect(out["lam"][:calls], 0.0)
    assert rise <= ref.tau_lam[:calls].max(), "%s: a Ritz value rose by %.3e of the block's largest" % (what, rise)


def _check_block(w, what, p, ref, out, k):
    """the whole block X_k: +-0.0 on the fixed variables, every cluster of the reference and the whole span; orthogonality to Z and Q"""
    X = out["X"]
    assert np.all(np.isfinite(X)) and np.all(X[:, p.mask] == 0.0), what + ": fixed rows"
    Xf = X[:, p.free].T
    e_sub = LU.measures(p, ref, k, out["lam"][k], out["res"][k], Xf)[2]
    w.sub = max(w.sub, e_sub / ref.tau_sub[k])
    assert e_sub <= ref.tau_sub[k], "%s: the block at k = %d off by %.3e > %.1e" % (what, k, e_sub, ref.tau_sub[k])
    for name, against in (("Z", p.Z), ("Q", p.Q)):
        if against is None:
            continue
        Bn = U.m_orthonormalise(against, p.B) if name == "Z" else against
        cosines = np.abs((p.B @ Bn).T @ Xf) / np.sqrt(np.sum(Xf * (p.B @ Xf), axis=0))[None, :]
        w.extra = max(w.extra, cosines.max() / ref.tau_sub[k])
        assert cosines.max() <= ref.tau_sub[k], "%s: |%s^T B X_%d| = %.3e > %.1e" % (what, name, k, cosines.max(), ref.tau_sub[k])


def _walk_case(case, precond="jacobi", ks=None):
    p = LU.problem(case)
    ks = case.ks if ks is None else ks
    hook = precond != "jacobi"
    what = "%s %s" % (LU.case_name(case), precond)
    c = _context(case, precond, HOOK_OPTIONS if hook else ())
    w = _Worst()
    try:
        kmax = max(ks)
        long_run = _run(c, case, p, kmax)
        assert long_run["precondUsed"] == PRECONDS[precond], "%s: the loop ran preconditioner %d" % (what, long_run["precondUsed"])
        if hook:
            ref = LU.reference(case, LU.hook_T(p, lambda r: c.debug_apply_precond(r)[0]), kmax, LU.TAU_HOOK)
            worst_gap = max(ref.gap_lam.max(), ref.gap_res.max(), ref.gap_sub.max())
            assert worst_gap <= LU.FLOOR_MAX, "%s: the reference's own floor %.2e: replace this input" % (what, worst_gap)
            assert min(ref.pivots) >= LU.PIVOT_MIN
        else:
            ref = LU.jacobi_reference(case)
        assert ref.restarts == 0 and long_run["iterations"] == -1
        _check_history(w, what, p, ref, long_run, kmax + 1)
        for k in ks:
            out = long_run if k == kmax else _run(c, case, p, k)
            assert out["iterations"] == -1 and out["sets"][k][2] == 0
            _check_block(w, what, p, ref, out, k)
    finally:
        c.close()
    print("%s: m %d, k in %s; %s; reference floors lam %.1e res %.1e subspace %.1e" % (
        what, p.m, tuple(ks), w, ref.gap_lam.max(), ref.gap_res.max(), ref.gap_sub.max()))


# ------------------------------------------------------------------------------------------------ a. vibration, clamped
@pytest.mark.parametrize("case", LU.CLAMPED + LU.DENSITY, ids=LU.case_name)
def test_clamped_vibration_iterates(case):
    _walk_case(case)


@pytest.mark.parametrize("precond", ["two-level", "multigrid"])
@pytest.mark.parametrize("case", LU.CLAMPED, ids=LU.case_name)
def test_clamped_vibration_iterates_under_a_hierarchy(case, precond):
    _walk_case(case, precond, LU.HOOK_KS)


# ------------------------------------------------------------------------------------------------ b - f
@pytest.mark.parametrize("case", LU.FREE_BODY, ids=LU.case_name)
def test_free_body_iterates(case):
    _walk_case(case)


@pytest.mark.parametrize("case", LU.FULL_BLOCK, ids=LU.case_name)
def test_full_block_iterates(case):
    assert LU.problem(case).m == LU.BLK_MAXC
    _walk_case(case)


@pytest.mark.parametrize("case", LU.BUCKLING, ids=LU.case_name)
def test_buckling_iterates(case):
    lam = np.asarray(LU.jacobi_reference(case).lam, dtype=float)
    # the random field: both signs in the Rayleigh-Ritz of the start block; Kg has far more than m negative directions, so from the first
    # iteration on the m smallest Ritz values are all negative, as every one is under axial compression
    assert lam.max() < 0 if case.field == "axial" else (lam[0].min() < 0 < lam[0].max() and lam[1:].max() < 0)
    _walk_case(case)


@pytest.mark.parametrize("case", LU.PRESTRESSED, ids=LU.case_name)
def test_prestressed_iterates(case):
    _walk_case(case)


@pytest.mark.parametrize("case", LU.DEFLATED, ids=LU.case_name)
def test_deflated_iterates(case):
    _walk_case(case)


# ------------------------------------------------------------------------------------------------ g. the stop and the soft lock
@pytest.mark.parametrize("precond", ["jacobi", "multigrid"])
@pytest.mark.parametrize("case", LU.STOP, ids=LU.case_name)
def test_stop_and_soft_lock(case, precond):
    p = LU.problem(case)
    what = "%s %s" % (LU.case_name(case), precond)
    c = _context(case, precond, HOOK_OPTIONS)
    w = _Worst()
    try:
        if precond == "jacobi":
            rtol, ref = LU.jacobi_stop(case)
        else:
            rtol, ref = LU.find_stop(case, LU.hook_T(p, lambda r: c.debug_apply_precond(r)[0]), LU.TAU_HOOK)
            worst_gap = max(ref.gap_lam.max(), ref.gap_res.max(), ref.gap_sub.max())
            assert worst_gap <= LU.FLOOR_MAX, "%s: the reference's own floor %.2e: replace this input" % (what, worst_gap)
        k_stop, locked_before, margin = LU.stop_margin(ref, rtol)
        assert margin >= 2.0 and locked_before >= 1 and min(ref.pivots) >= LU.PIVOT_MIN and ref.restarts == 0
        out = _run(c, case, p, LU.STOP_ITERS, rtol)
        assert out["precondUsed"] == PRECONDS[precond]
        assert out["iterations"] == k_stop, "%s: stopped at %d, the reference at %d (rtol %.3g)" % (what, out["iterations"], k_stop, rtol)
        _check_history(w, what, p, ref, out, k_stop + 1)          # (|W| and |P| per iteration: the unconverged columns alone)
        assert np.all(out["sets"][k_stop + 1:] == -1) and np.all(np.isnan(out["lam"][k_stop + 1:]))
        _check_block(w, what, p, ref, out, k_stop)          # (locked columns included: they moved through Rayleigh-Ritz alone)
        again = _run(c, case, p, LU.STOP_ITERS, rtol)
        for name in ("X", "lam", "res", "sets"):
            assert np.array_equal(out[name], again[name], equal_nan=name != "sets"), "%s: %s differs between two calls under deterministic 1" % (what, name)
    finally:
        c.close()
    print("%s: rtol %.3g, k* %d, %d columns locked before it, margin %.2f, sets %s; %s" % (what, rtol, k_stop, locked_before, margin, ref.sets, w))


# ------------------------------------------------------------------------------------------------ h. the space runs out
def _two_triangles(fixed):
    V = np.array([[0.0, 0.0], [1.0, 0.0], [1.1, 0.9], [-0.1, 1.0]])
    T = np.array([[0, 1, 2], [0, 2, 3]])
    m = O.FEMMesh(T, V, 1)
    sim = O.Simulator(T, V, 1, mesh=m)
    sim.set_material_constant(O.ElasticityTensor.isotropic(2, U.E_MOD, U.NU))
    K = sp.csr_matrix(sim.assembleStiffnessMatrix().sum_repeated().to_scipy_full_from_upper())
    Mm = sp.csr_matrix(sp.kron(O.mass_triplets(m).sum_repeated().to_scipy_full_from_upper(), sp.identity(2)))
    free = np.setdiff1d(np.arange(8), fixed)
    lam = scipy.linalg.eigh(K[free][:, free].toarray(), Mm[free][:, free].toarray(), eigvals_only=True)
    c = M.Context(0)
    c.mesh_build(T, V, 1)
    c.material_isotropic(U.E_MOD, U.NU)
    c.set_preconditioner(M.PRECOND_BLOCK_JACOBI)
    c.fix_variables(np.asarray(fixed, dtype=np.int64))
    assert np.array_equal(c.node_positions(), np.asarray(m.node_pos))
    return c, lam


def test_start_block_spans_the_space():
    c, lam = _two_triangles([0, 1, 2, 3])          # nEff = 4, nev = 2: m = 4 = nEff
    try:
        assert c.debug_lobpcg_block_size("vibration", 2) == 4
        S0 = np.random.default_rng(3).standard_normal((4, 8))
        out = c.debug_lobpcg("vibration", S0, 2, rtol=1e-10, maxit=3)
        assert out["iterations"] == 0 and tuple(out["sets"][0]) == (0, 0, 0)
        err = np.abs(out["lam"][0] - lam).max() / lam.max()
        print("nEff = m = 4: Rayleigh-Ritz of the start against eigh %.1e, residuals %s" % (err, out["res"][0]))
        assert err <= 1e-13
        with pytest.raises(M.MeshFEMHipError) as ei:          # a start block of another row count is refused
            c.debug_lobpcg("vibration", S0[:3], 2)
        assert ei.value.code == _lib.ERR_INVALID
    finally:
        c.close()


def test_directions_run_out():
    c, lam = _two_triangles([0, 1, 3])          # nEff = 5, m = 4: W has rank 1
    try:
        assert c.debug_lobpcg_block_size("vibration", 2) == 4
        S0 = np.random.default_rng(4).standard_normal((4, 8))
        out = c.debug_lobpcg("vibration", S0, 2, rtol=1e-30, maxit=1)
        assert tuple(out["sets"][1]) == (1, 0, 0), "|W|, |P|, restarts = %s" % (out["sets"][1],)
        err = np.abs(out["lam"][1] - lam[:4]).max() / lam[:4].max()
        print("nEff = 5, m = 4: three columns of W dropped; after one iteration against eigh %.1e" % err)
        assert err <= 1e-13
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ i. the public entry point
@pytest.mark.parametrize("k", [1, 3])
def test_public_warm_start_runs_k_iterations(k):
    case = LU.PRESTRESSED[0]
    p = LU.problem(case)
    c = _context(case)
    try:
        with pytest.raises(M.MeshFEMHipError) as ei:
            c.modes_prestressed(case.nev, _load_factor(case), x0=p.S0[:case.nev], rtol=1e-30, maxit=k)
        assert ei.value.code == _lib.ERR_NOT_CONVERGED
        lam, X, info = c.last_modes_prestressed
        assert info["iterations"] == k and info["converged"] == 0
        assert np.all(np.isfinite(lam)) and np.all(np.isfinite(X)) and np.all(np.isfinite(info["residuals"]))
    finally:
        c.close()
