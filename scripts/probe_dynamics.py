"""Record of the Newmark time stepper on one MI355X: BASELINE configs[2] (60^3 quadratic tets) clamped on the face x = 0, loaded on x = 1, 20 steps at
dt = T_1 / 20 and T_1 / 200 (T_1 from mfh_modes), rtol 1e-8, block-Jacobi and multigrid. Writes profiles/r09_dynamics.md (or --out): time per step,
PCG iterations per step, time per PCG iteration, and that last figure against its floor -- the per-iteration time of mfh_solve on the same context
with the same preconditioner plus one k_spmv_kron product (mfh_time_spmv_kernel under MFH_OP_MASS_VECTOR) -- with a per-phase breakdown from one
further run with a synchronisation at every phase boundary (MFH_DYN_TIMING)."""
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


PHASES = ["K product", "M product (k_spmv_kron_acc) + p.Ap", "residual update (+ block-Jacobi)", "coarse preconditioner + r.z", "direction",
          "read-back of the history (synchronisation)", "step kernels (predict, right-hand side, correct)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60, help="grid cells per axis (BASELINE configs[2]: 60)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r09_dynamics.md"))
    a = ap.parse_args()
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(a.n, a.n, a.n, [0, 0, 0], [1, 1, 1])
    cm = M.Context(0)
    cm.set_option("matrix_storage", 0)
    cm.mesh_build(T, V, 2)
    cm.set_operator(M.OP_MASS_VECTOR)
    cm.assemble()
    m_ms = cm.time_spmv_kernel(reps=20)
    cm.close()
    lines = ["# Newmark time stepping on one MI355X: %d^3 quadratic tets, clamped on x = 0, %d steps, rtol %g" % (a.n, a.steps, a.rtol), ""]
    rows, breakdowns, best, ratios = [], [], {}, []
    t1 = None
    for pname, pre in (("block-Jacobi", M.PRECOND_BLOCK_JACOBI), ("multigrid", M.PRECOND_MULTIGRID)):
        c = M.Context(0)
        c.set_option("matrix_storage", 0)          # both triangles from the start: the calls do not re-run the symbolic phase
        c.mesh_build(T, V, 2)
        c.material_isotropic(1.0, 0.3)
        c.set_preconditioner(pre)
        c.bc_dirichlet_box([-1e-9, -1e9, -1e9], [1e-9, 1e9, 1e9], [0, 0, 0])
        fixed, _ = c.bc_dirichlet_vars()
        c.fix_variables(fixed)
        n = c.bs * c.n_dof
        if t1 is None:
            lines += ["%d elements, %d unknowns (%d fixed)." % (c.n_elem, n, len(fixed)), ""]
        f = np.zeros(n)
        f[1::3] = -1.0 / n
        k_ms = c.time_spmv_kernel(reps=20)
        c.solve(f, rtol=1e-6)                       # warm-up (hierarchy, lists)
        c.solve(f, rtol=1e-6)
        pcg_iter_ms = c.last_info["solve_ms"] / max(1, c.last_info["iterations"])
        if t1 is None:
            c.set_preconditioner(M.PRECOND_MULTIGRID)
            lam, _, _ = c.modes(1, rtol=1e-6, maxit=500)
            c.set_preconditioner(pre)
            t1 = 2.0 * np.pi / np.sqrt(lam[0])
            lines += ["T_1 = %.6g (lambda_1 = %.6g from mfh_modes, density 1). M product (k_spmv_kron, mfh_time_spmv_kernel): %.3f ms." % (t1, lam[0], m_ms), ""]
        floor = pcg_iter_ms + m_ms
        for frac in (20, 200):
            dt = t1 / frac
            c.newmark(dt, 2, f=f, rtol=a.rtol, maxit=20000)                  # warm-up
            r = c.newmark(dt, a.steps, f=f, rtol=a.rtol, maxit=20000)
            info = r["info"]
            its = info["iterationsTotal"]
            per_it = info["solve_ms"] / max(1, its + info["iterationsInit"])
            os.environ["MFH_DYN_TIMING"] = "1"
            (rt, err) = _capture_stderr(lambda: c.newmark(dt, max(2, a.steps // 4), f=f, rtol=a.rtol, maxit=20000))
            del os.environ["MFH_DYN_TIMING"]
            mt = re.search(r"ms: K ([\d.]+) M ([\d.]+) update ([\d.]+) precond ([\d.]+) direction ([\d.]+) readback ([\d.]+) step-kernels ([\d.]+)", err)
            ph = [float(x) for x in mt.groups()] if mt else [float("nan")] * 7
            itt = max(1, rt["info"]["iterationsTotal"] + rt["info"]["iterationsInit"])
            ratios.append((pname, frac, per_it / floor, [p / itt for p in ph], m_ms, k_ms, pcg_iter_ms))
            rows.append("| %s | T_1 / %d | %.2f | %.1f | %d | %.3f | %.3f | %.3f | %.3f | **%.2f** |" %
                        (pname, frac, info["solve_ms"] / a.steps, its / a.steps, info["iterationsMax"], per_it, pcg_iter_ms, k_ms, floor, per_it / floor))
            breakdowns.append((pname, frac, [p / itt for p in ph], rt["info"]["solve_ms"] / itt))
            best.setdefault(frac, []).append((info["solve_ms"] / a.steps, pname))
        c.close()
    lines += ["## Per step and per PCG iteration", "",
              "solve_ms of the call (device events around the time loop; the solve for a0 included) over the steps; iterations of the steps alone.",
              "Floor = one PCG iteration of mfh_solve on the same context and preconditioner (rtol 1e-6, second solve) + one k_spmv_kron product.", "",
              "| preconditioner | dt | ms per step | iterations per step | worst step | ms per iteration | mfh_solve ms per iteration | K product ms | floor ms | ratio to the floor |",
              "|---|---|---|---|---|---|---|---|---|---|"] + rows + [""]
    lines += ["## Where an iteration goes", "",
              "One further run per case (a quarter of the steps) with a stream synchronisation at every phase boundary (the phases add up to more than the free-running call).", "",
              "| preconditioner | dt | " + " | ".join(PHASES) + " | sum, synchronised |", "|---|---|" + "---|" * (len(PHASES) + 1)]
    for pname, frac, ph, tot in breakdowns:
        lines.append("| %s | T_1 / %d | " % (pname, frac) + " | ".join("%.3f" % p for p in ph) + " | %.3f |" % tot)
    lines += ["", "(ms per PCG iteration; the step kernels and the read-back are per-step costs spread over the step's iterations.)", "",
              "## Reading the ratio", "",
              "The allowance is 1.3: a loop without graph capture and one extra vector sweep. Per case, what the synchronised phases take beyond their"
              " counterparts in the floor (M phase against k_spmv_kron alone; K phase against the timed K product; everything else against the rest of an"
              " mfh_solve iteration):", ""]
    for pname, frac, ratio, ph, mm, kk, pit in ratios:
        other = ph[2] + ph[3] + ph[4] + ph[5] + ph[6]
        lines.append("- %s, T_1 / %d: ratio %.2f (%s 1.3); M phase %+.3f ms, K phase %+.3f ms, vector kernels + preconditioner + per-step work %+.3f ms" %
                     (pname, frac, ratio, "above" if ratio > 1.3 else "within", ph[1] - mm, ph[0] - kk, other - (pit - kk)))
    lines += ["", "## Which preconditioner", ""]
    for frac in (20, 200):
        w = min(best[frac])
        lines.append("- dt = T_1 / %d: %s (%s)" % (frac, w[1], ", ".join("%s %.2f ms per step" % (p, t) for t, p in sorted(best[frac]))))
    lines += ["", "## Next to measure", "",
              "A matrix-free mass product. The assembled M product (k_spmv_kron / k_spmv_kron_acc, %.3f ms) costs about three times the matrix-free K product"
              " and now sits inside every PCG iteration of every step; the element mass matrix is a constant table times the element volume, so a"
              " cluster kernel like the K operator's would read the vertex positions instead of 12 bytes per stored block." % m_ms, ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
