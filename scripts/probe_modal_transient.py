"""Record of the modal transient response on one MI355X: the setup of scripts/probe_modal.py (BASELINE configs[2], 60^3 quadratic tets, clamped on the
face x = 0, 64 modes by mfh_modes_many, the Rayleigh case 0.1 omega_1 / 0.02 / omega_1), a step load from rest. Writes
profiles/r19_modal_transient.md (or --out):
  - k_modal_series against the k_modal_expand route on the gathered probe rows (mfh_time_modal_series), the two taking turns, --rounds rounds:
    the acceptance figure of the series kernel
  - --steps steps (100 000) with two probes only: march / series / total ms, for chunkSteps in {256, 1 024, 4 096, 16 384} (the sweep the default
    is taken from)
  - the same with 100 snapshots
  - the cost per step beside one mfh_newmark step, rerun in this process at dt = T_1 / 20 with the multigrid preconditioner (the case of
    profiles/r09_dynamics.md)
  - the distance of the probe histories from a --newmark-steps step (2 000) Newmark run at the same dt, with and without the static correction
Every timed call is preceded by a warm-up call of the same shape."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60, help="grid cells per axis (BASELINE configs[2]: 60)")
    ap.add_argument("--modes", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100000)
    ap.add_argument("--snapshots", type=int, default=100)
    ap.add_argument("--newmark-steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--maxit", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r19_modal_transient.md"))
    a = ap.parse_args()
    import meshfem_amd as M
    from meshfem_amd import grid
    lines = ["# Modal transient response on one MI355X: %d^3 quadratic tets, clamped on x = 0, %d modes, Rayleigh damping (0.1 omega_1, 0.02 / omega_1)" % (a.n, a.modes), ""]

    def say(*ls):
        lines.extend(ls)
        print("\n".join(ls), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    V, T = grid.grid_tet_mesh(a.n, a.n, a.n, [0, 0, 0], [1, 1, 1])
    c = M.Context(0)
    c.set_option("matrix_storage", 0)          # both triangles from the start: the calls do not re-run the symbolic phase
    c.mesh_build(T, V, 2)
    c.material_isotropic(1.0, 0.3)
    c.set_preconditioner(M.PRECOND_MULTIGRID)
    c.bc_dirichlet_box([-1e-9, -1e9, -1e9], [1e-9, 1e9, 1e9], [0, 0, 0])
    fixed, _ = c.bc_dirichlet_vars()
    c.fix_variables(fixed)
    n = c.bs * c.n_dof
    f = np.zeros(n)
    f[1::3] = -1.0 / n
    c.solve(f, rtol=1e-6)                       # warm-up (hierarchy, lists)
    say("%d elements, %d unknowns (%d fixed)." % (c.n_elem, n, len(fixed)), "")

    # ---- the series kernel against the expansion kernel on the gathered rows
    say("## k_modal_series against the k_modal_expand route, %d modes" % a.modes, "",
        "%d rounds; in each the two take turns, 3 launches each (one event pair per launch; the expand route is one launch per 32 steps inside the pair)." % a.rounds,
        "Median [min, max] in ms.", "", "| probes | steps | k_modal_series | k_modal_expand route | series / expand |", "|---|---|---|---|---|")
    verdicts = []
    for n_probe, steps in ((2, 4096), (2, a.steps), (17, a.steps)):
        s, e = [], []
        for _ in range(a.rounds):
            ts, te = c.time_modal_series(a.modes, n_probe, steps, reps=3)
            s.extend(ts)
            e.extend(te)
        s, e = np.array(s), np.array(e)
        spread = max(s.max() - s.min(), e.max() - e.min())
        verdicts.append(np.median(s) <= np.median(e) + spread)
        say("| %d | %d | %.4f [%.4f, %.4f] | %.4f [%.4f, %.4f] | %.3f |" % (n_probe, steps, np.median(s), s.min(), s.max(), np.median(e), e.min(), e.max(), np.median(s) / np.median(e)))
    say("", "Acceptance: the series kernel is %s beyond the run-to-run range of these rounds." % ("not slower" if all(verdicts) else "SLOWER in at least one shape"), "")

    # ---- the basis
    t0 = time.time()
    lam, X, info = c.modes_many(a.modes, batch=16, rtol=1e-6, maxit=3000)
    t_modes = time.time() - t0
    w1 = float(np.sqrt(lam[0]))
    bi = c.set_modal_basis(lam, X)
    del X
    say("## The basis", "", "modes_many(%d): %.1f s wall; set_modal_basis %.0f ms; omega_1 = %.6g, omega_%d = %.6g." % (a.modes, t_modes, bi["setupMs"], w1, a.modes, float(np.sqrt(lam[-1]))), "")
    damping = (0.1 * w1, 0.02 / w1)
    dt = 2.0 * np.pi / w1 / 20.0
    probes = [n - 2, n // 2]

    # ---- the long run, probes only: the chunk sweep
    say("## %d steps at dt = T_1 / 20, two probes, static correction" % a.steps, "",
        "| chunkSteps | wall s | setupMs (load, Gram, static solve) | marchMs | seriesMs | march us per step | chunks |", "|---|---|---|---|---|---|---|")
    c.modal_transient(dt, 1000, f, damping=damping, rtol=a.rtol, maxit=a.maxit, probes=probes)            # warm-up
    ref, worst = None, 0.0
    for chunk in (256, 1024, 4096, 16384, 0):
        t0 = time.time()
        r = c.modal_transient(dt, a.steps, f, damping=damping, rtol=a.rtol, maxit=a.maxit, probes=probes, chunk_steps=chunk)
        wall = time.time() - t0
        i = r["info"]
        say("| %s | %.3f | %.1f | %.2f | %.2f | %.3f | %d |" % ("%d" % chunk if chunk else "default (%d)" % i["chunkSteps"], wall, i["setupMs"], i["marchMs"], i["seriesMs"],
                                                          1e3 * i["marchMs"] / a.steps, i["chunks"]))
        if ref is None:
            ref = r["probes"]
        else:
            worst = max(worst, float(np.abs(r["probes"] - ref).max() / np.abs(ref).max()))
    say("", "(Every call makes its own static solve at rtol %g with sums in arrival order: the probe histories of these calls differ by %.1e of their maximum at most;" % (a.rtol, worst),
        "under option deterministic they are identical bit for bit at every chunk length, tests/test_gpu_modal_transient.py.)", "")

    # ---- with snapshots
    stride = max(1, a.steps // a.snapshots)
    t0 = time.time()
    r = c.modal_transient(dt, a.steps, f, damping=damping, rtol=a.rtol, maxit=a.maxit, probes=probes, snapshot_stride=stride)
    wall = time.time() - t0
    i = r["info"]
    say("## The same with %d snapshots (%.1f GB on the host)" % (len(r["snapshots"]), r["snapshots"].nbytes / 1e9), "",
        "wall %.2f s: setupMs %.1f, marchMs %.2f, seriesMs %.2f, expandMs %.2f (the copies to the host are the rest)." % (wall, i["setupMs"], i["marchMs"], i["seriesMs"], i["expandMs"]), "")
    assert np.array_equal(r["probes"][::stride][:, 0], r["snapshots"][:, probes[0]])
    del r

    # ---- beside mfh_newmark
    c.newmark(dt, 2, f=f, damping=damping, rtol=a.rtol, maxit=a.maxit)                                       # warm-up
    t0 = time.time()
    nm_probes, state, solve_ms, block = [], {}, 0.0, 250          # in blocks chained through (u, v, a): the same run, with a sign of life in between
    for s0 in range(0, a.newmark_steps, block):
        k = min(block, a.newmark_steps - s0)
        nm = c.newmark(dt, k, f=f, damping=damping, rtol=a.rtol, maxit=a.maxit, probes=probes, **state)
        state = dict(u0=nm["u"], v0=nm["v"], a0=nm["a"])
        nm_probes.append(nm["probes"] if s0 == 0 else nm["probes"][1:])
        solve_ms += nm["info"]["solve_ms"]
        print("newmark: %d steps done" % (s0 + k), flush=True)
    nm_probes = np.concatenate(nm_probes)
    t_nm = time.time() - t0
    say("## Beside mfh_newmark (multigrid, rtol %g, dt = T_1 / 20, %d steps)" % (a.rtol, a.newmark_steps), "",
        "mfh_newmark: %.1f s wall, %.1f ms per step (solve_ms over the steps)." % (t_nm, solve_ms / max(1, a.newmark_steps)), "",
        "| static correction | max_n |probe_modal - probe_newmark| / max_n |probe_newmark| |", "|---|---|")
    for corrected in (True, False):
        r = c.modal_transient(dt, a.newmark_steps, f, damping=damping, rtol=a.rtol, maxit=a.maxit, probes=probes, static_correction=corrected)
        d = np.abs(r["probes"] - nm_probes).max(axis=0) / np.abs(nm_probes).max(axis=0)
        say("| %s | %.3e, %.3e |" % ("yes" if corrected else "no", d[0], d[1]))
    say("", "(Newmark's own period error at 20 steps per period of mode 1 is part of the distance; the modal run has none.)", "")
    c.close()


if __name__ == "__main__":
    main()
