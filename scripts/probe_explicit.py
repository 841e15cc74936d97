"""Record of the explicit stepper on one MI355X: BASELINE configs[2] (60^3 quadratic tets) clamped on the face x = 0, loaded on x = 1, 1 000 steps of
mfh_explicit at 0.9 dtEst. Writes profiles/r17_explicit.md (or --out): ms per step, its split into the K product and k_explicit_step, and the
floor -- the K product timed in the same process (mfh_time_spmv_kernel) plus a device-to-device copy of the bytes the step kernel must move (five
reads and two writes per variable, mfh_time_explicit_step) --, the time of mfh_explicit_dt, and the simulated time per wall second against
mfh_newmark at dt = T_1 / 200 with block-Jacobi (its better preconditioner there, profiles/r09_dynamics.md)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60, help="grid cells per axis (BASELINE configs[2]: 60)")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--newmark-steps", type=int, default=8, help="0: skip the comparison with mfh_newmark")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r17_explicit.md"))
    a = ap.parse_args()
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(a.n, a.n, a.n, [0, 0, 0], [1, 1, 1])

    def context(storage=None):
        c = M.Context(0)
        if storage is not None:
            c.set_option("matrix_storage", storage)
        c.mesh_build(T, V, 2)
        c.material_isotropic(1.0, 0.3)
        c.bc_dirichlet_box([-1e-9, -1e9, -1e9], [1e-9, 1e9, 1e9], [0, 0, 0])
        fixed, _ = c.bc_dirichlet_vars()
        c.fix_variables(fixed)
        return c, len(fixed)
    c, n_fixed = context()
    n = c.bs * c.n_dof
    f = np.zeros(n)
    f[1::3] = -1.0 / n
    lines = ["# Explicit central differences on one MI355X: %d^3 quadratic tets, clamped on x = 0, %d steps" % (a.n, a.steps), "",
             "%d elements, %d unknowns (%d fixed). Default context: matrix-free cluster operator, upper-triangle storage kept." % (c.n_elem, n, n_fixed), ""]
    c.explicit_dt()                                     # warm-up: geometry, lists, K
    lim = [c.explicit_dt() for _ in range(3)]
    dt = 0.9 * lim[-1]["dtEst"]
    lines += ["## The stable step", "",
              "mfh_explicit_dt (Gershgorin bound + 60 power-iteration steps), three calls after a warm-up: %s ms." % ", ".join("%.2f" % x["ms"] for x in lim),
              "lambdaUpper %.6g, lambdaEst %.6g: dtSafe %.6g, dtEst %.6g (ratio %.3f). The run below takes dt = 0.9 dtEst = %.6g." %
              (lim[-1]["lambdaUpper"], lim[-1]["lambdaEst"], lim[-1]["dtSafe"], lim[-1]["dtEst"], lim[-1]["dtSafe"] / lim[-1]["dtEst"], dt), ""]
    k_ms = [c.time_spmv_kernel(reps=50) for _ in range(3)]
    step_copy = [c.time_explicit_step(n, reps=50) for _ in range(3)]
    c.explicit(dt, 50, f=f, check_dt=False)             # warm-up
    runs = [c.explicit(dt, a.steps, f=f, check_dt=False)["info"] for _ in range(3)]
    per_step = sorted(r["solve_ms"] / a.steps for r in runs)
    probed = c.explicit(dt, a.steps, f=f, check_dt=False, probes=[n - 1, n // 2], energies=True, energy_stride=10)["info"]["solve_ms"] / a.steps
    k_med, s_med, c_med = sorted(k_ms)[1], sorted(x[0] for x in step_copy)[1], sorted(x[1] for x in step_copy)[1]
    floor = k_med + c_med
    lines += ["## Per step", "",
              "solve_ms of the call (device events around the time loop: %d launches of the K product and of k_explicit_step, a flag read every 256 steps) over the steps;"
              " three runs after a warm-up, all listed. The parts are timed alone in the same process, three times each (median taken): the K product by"
              " mfh_time_spmv_kernel, k_explicit_step and the copy of the bytes it moves (3.5 n doubles read and written) by mfh_time_explicit_step." % (a.steps + 1), "",
              "| ms per step (three runs) | K product ms | k_explicit_step ms | copy of its bytes ms | floor = K + copy ms | ratio to the floor (median run) |",
              "|---|---|---|---|---|---|",
              "| %s | %s | %s | %s | %.3f | **%.2f** |" % (", ".join("%.3f" % x for x in per_step), ", ".join("%.3f" % x for x in k_ms),
                                                          ", ".join("%.3f" % x[0] for x in step_copy), ", ".join("%.3f" % x[1] for x in step_copy), floor, per_step[1] / floor), "",
              "K + k_explicit_step timed alone: %.3f ms; the free-running step: %.3f ms. With two probes and an energy row every 10 steps: %.3f ms per step." %
              (k_med + s_med, per_step[1], probed), "",
              "The allowance is the 1.3 of docs/design/04_13_dynamics.md: the ratio is %s it." % ("within" if per_step[1] / floor <= 1.3 else "ABOVE"), ""]
    c.close()
    if a.newmark_steps > 0:
        cw, _ = context(0)
        cw.set_preconditioner(M.PRECOND_MULTIGRID)
        lam, _, _ = cw.modes(1, rtol=1e-6, maxit=500)
        t1 = 2.0 * np.pi / np.sqrt(lam[0])
        cw.set_preconditioner(M.PRECOND_BLOCK_JACOBI)
        dtn = t1 / 200
        cw.newmark(dtn, 2, f=f, rtol=1e-8, maxit=20000)
        info = cw.newmark(dtn, a.newmark_steps, f=f, rtol=1e-8, maxit=20000)["info"]
        cw.close()
        nm_ms = info["solve_ms"] / a.newmark_steps
        lines += ["## Simulated time per wall second", "",
                  "T_1 = %.6g (mfh_modes). mfh_newmark at dt = T_1 / 200 = %.6g, block-Jacobi, rtol 1e-8, %d steps: %.1f ms per step (%.1f PCG iterations per step)." %
                  (t1, dtn, a.newmark_steps, nm_ms, info["iterationsTotal"] / a.newmark_steps), "",
                  "| scheme | dt | ms per step | simulated time per wall second |", "|---|---|---|---|",
                  "| mfh_explicit | %.6g | %.3f | %.4g |" % (dt, per_step[1], dt / per_step[1] * 1e3),
                  "| mfh_newmark | %.6g | %.1f | %.4g |" % (dtn, nm_ms, dtn / nm_ms * 1e3), "",
                  "Explicit steps are %.0f times shorter than T_1 / 200 and %.0f times cheaper: %.2f times the simulated time per wall second. The explicit scheme is"
                  " the one to take where the step is set by accuracy at the mesh's own time scale (waves, impact), the implicit one where the response is slow." %
                  (dtn / dt, nm_ms / per_step[1], (dt / per_step[1]) / (dtn / nm_ms)), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
