"""Record of the frequency-response solver on one MI355X: BASELINE configs[2] (60^3 quadratic tets) clamped on the face x = 0, the Rayleigh case
(0.1 omega_1, 0.02 / omega_1; omega_1 from mfh_modes), rtol 1e-8, omega in {0.5, 1.5, 3} omega_1, block-Jacobi and multigrid. Writes
profiles/r13_harmonic.md (or --out):
  - ms per complex COCG iteration against 2 x the per-iteration time of mfh_newmark's PCG with the same preconditioner in the same process
  - the complex mass product in one pass (k_spmv_kron_cacc) against two launches of k_spmv_kron_acc + k_harm_combine (option harmonic_two_pass):
    the loop's ms per iteration both ways, and the M phase alone from runs with a synchronisation at every phase boundary (MFH_DYN_TIMING)
  - iterations per frequency for both preconditioners
Every timed call is preceded by a warm-up call of the same shape; times are device events around the sweep (info["solveMs"])."""
import argparse
import os
import re
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _capture_stderr(fn):
    """fn() with the process's stderr (the C library writes there) captured."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


PHASES = ["K products (two planes)", "M product + p^T Z p", "residual update (+ block-Jacobi)", "coarse preconditioner (two planes) + r^T z", "direction",
          "read-back of the history (synchronisation)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60, help="grid cells per axis (BASELINE configs[2]: 60)")
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--maxit", type=int, default=20000)
    ap.add_argument("--timing-iterations", type=int, default=40, help="iterations of the synchronised runs (they stop at maxit on purpose)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r13_harmonic.md"))
    a = ap.parse_args()
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(a.n, a.n, a.n, [0, 0, 0], [1, 1, 1])
    lines = ["# Frequency response on one MI355X: %d^3 quadratic tets, clamped on x = 0, Rayleigh damping (0.1 omega_1, 0.02 / omega_1), rtol %g" % (a.n, a.rtol), ""]
    w1 = None
    rows, phase_rows, it_rows, verdicts = [], [], [], []

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines + report()))

    def report():
        out = ["## Per complex iteration", "",
               "solveMs of the call (device events around the sweep, the true-residual products included) over its iterations. Newmark: solve_ms of 5 steps at",
               "dt = T_1 / 20 with the same preconditioner over their PCG iterations (the solve for a0 included), same process.", "",
               "| preconditioner | mass product | ms per complex iteration | Newmark ms per PCG iteration | ratio to 2 x Newmark |", "|---|---|---|---|---|"] + rows + [""]
        out += ["## Where a complex iteration goes", "",
                "Runs of %d iterations at 1.5 omega_1 with a stream synchronisation at every phase boundary (ms per iteration; the phases add up to more than" % a.timing_iterations,
                "the free-running call). The Newmark row is its own MFH_DYN_TIMING run: its M phase is ONE launch of k_spmv_kron_acc, so two launches cost twice it.", "",
                "| preconditioner | loop | " + " | ".join(PHASES) + " |", "|---|---|" + "---|" * len(PHASES)] + phase_rows + [""]
        out += ["## Iterations per frequency", "", "| preconditioner | omega / omega_1 | iterations (warm start in sweep order) | true residual |", "|---|---|---|---|"] + it_rows + [""]
        out += ["## Verdicts", ""] + verdicts + [""]
        return out

    for pname, pre in (("multigrid", M.PRECOND_MULTIGRID), ("block-Jacobi", M.PRECOND_BLOCK_JACOBI)):
        c = M.Context(0)
        c.set_option("matrix_storage", 0)          # both triangles from the start: the calls do not re-run the symbolic phase
        c.mesh_build(T, V, 2)
        c.material_isotropic(1.0, 0.3)
        c.set_preconditioner(pre)
        c.bc_dirichlet_box([-1e-9, -1e9, -1e9], [1e-9, 1e9, 1e9], [0, 0, 0])
        fixed, _ = c.bc_dirichlet_vars()
        c.fix_variables(fixed)
        n = c.bs * c.n_dof
        f = np.zeros(n)
        f[1::3] = -1.0 / n
        c.solve(f, rtol=1e-6)                       # warm-up (hierarchy, lists)
        if w1 is None:
            lam, _, _ = c.modes(1, rtol=1e-6, maxit=500)
            w1 = float(np.sqrt(lam[0]))
            lines += ["%d elements, %d unknowns (%d fixed). omega_1 = %.6g (lambda_1 = %.6g from mfh_modes, density 1)." % (c.n_elem, n, len(fixed), w1, lam[0]), ""]
        damping = (0.1 * w1, 0.02 / w1)
        om = np.array([0.5, 1.5, 3.0]) * w1
        dt = 2.0 * np.pi / w1 / 20.0
        c.newmark(dt, 2, f=f, damping=damping, rtol=a.rtol, maxit=a.maxit)                  # warm-up
        nm = c.newmark(dt, 5, f=f, damping=damping, rtol=a.rtol, maxit=a.maxit)["info"]
        nm_it = nm["solve_ms"] / max(1, nm["iterationsTotal"] + nm["iterationsInit"])
        os.environ["MFH_DYN_TIMING"] = "1"
        (rt, err) = _capture_stderr(lambda: c.newmark(dt, 2, f=f, damping=damping, rtol=a.rtol, maxit=a.maxit))
        mt = re.search(r"ms: K ([\d.]+) M ([\d.]+) update ([\d.]+) precond ([\d.]+) direction ([\d.]+) readback ([\d.]+)", err)
        itt = max(1, rt["info"]["iterationsTotal"] + rt["info"]["iterationsInit"])
        nm_ph = [float(x) / itt for x in mt.groups()] if mt else [float("nan")] * 6
        del os.environ["MFH_DYN_TIMING"]
        phase_rows.append("| %s | Newmark PCG (real) | " % pname + " | ".join("%.3f" % p for p in nm_ph) + " |")
        per_it = {}
        for two_pass in (0, 1):
            form = "two launches + combine" if two_pass else "one pass (k_spmv_kron_cacc)"
            c.set_option("harmonic_two_pass", two_pass)
            c.harmonic(om[:1], f, damping=damping, rtol=1e-3, maxit=a.maxit, fields=False)      # warm-up
            r = c.harmonic(om, f, damping=damping, rtol=a.rtol, maxit=a.maxit, fields=False, probes=[n - 2])
            info = r["info"]
            per_it[two_pass] = info["solveMs"] / max(1, info["iterationsTotal"])
            rows.append("| %s | %s | %.3f | %.3f | **%.2f** |" % (pname, form, per_it[two_pass], nm_it, per_it[two_pass] / (2.0 * nm_it)))
            if not two_pass:
                for k in range(len(om)):
                    it_rows.append("| %s | %.1f | %d | %.2e |" % (pname, om[k] / w1, r["iterations"][k], r["true_residuals"][k]))
            os.environ["MFH_DYN_TIMING"] = "1"

            def timed():
                try:
                    c.harmonic(om[1:2], f, damping=damping, rtol=1e-14, maxit=a.timing_iterations, fields=False)
                except M.MeshFEMHipError:
                    pass                            # stops at maxit on purpose: the laps are what is wanted
            (_, err) = _capture_stderr(timed)
            del os.environ["MFH_DYN_TIMING"]
            mt = re.search(r"\[mfh_harmonic\].*ms: K ([\d.]+) M ([\d.]+) update ([\d.]+) precond ([\d.]+) direction ([\d.]+) readback ([\d.]+)", err)
            ph = [float(x) / a.timing_iterations for x in mt.groups()] if mt else [float("nan")] * 6
            phase_rows.append("| %s | COCG, %s | " % (pname, form) + " | ".join("%.3f" % p for p in ph) + " |")
            print("\n".join(rows[-1:] + phase_rows[-2:]), flush=True)
            flush()
        c.set_option("harmonic_two_pass", 0)
        ratio = per_it[0] / (2.0 * nm_it)
        verdicts.append("- %s: one complex iteration = %.2f x two Newmark PCG iterations (%s the allowance of 2 x with 5 %% spread); one pass %.3f ms, two passes %.3f ms per iteration: the single-pass kernel is %s." %
                        (pname, ratio, "within" if ratio <= 1.05 else "ABOVE", per_it[0], per_it[1], "faster" if per_it[0] < per_it[1] else "NOT faster"))
        c.close()
        flush()
    print("\n".join(lines + report()))


if __name__ == "__main__":
    main()
