"""Record of linear buckling on one MI355X (docs/design/04_16_buckling.md) on BASELINE configs[2] (60^3 grid -> quadratic tets), clamped on the face
x = min under the uniform prestress sigma_xx = -1:
  (a) the geometric-stiffness assembly pass (k_assemble_gather<3, 2, MAT_GEOM>) against the Laplacian pass (MAT_LAPLACE: the same H arithmetic, the
      code of the commit before the feature) and the unit-density mass pass (MAT_MASS) into the same buffer on the same context, launched in turns,
      device events per launch (mfh_time_geometric_assembly);
  (b) mfh_buckling, nev 4, multigrid: iterations, time, the split by phase (one run with a synchronisation at every phase boundary,
      MFH_MODES_TIMING) and the floor m (K product + Kg product + V-cycle) from mfh_time_spmv_kernel and the timers of a PCG solve on the same context
      (the Kg product is k_spmv_kron, timed as the MFH_OP_MASS_VECTOR product of a second context: the same kernel on the same pattern).
  (c) y = Kg x on a context with default options (upper-triangle storage: every call re-runs the symbolic phase and the assembly) against a
      context with option matrix_storage 0 (assembled once), host clock around the call.
Prints the measured section of profiles/r12_buckling.md (and writes it to --out if given); the tables of kernel resources in that file come from
the compiler, not from this script."""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60, help="grid cells per axis (BASELINE configs[2]: 60)")
    ap.add_argument("--nev", type=int, default=4)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=500)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--no-apply", action="store_true")
    ap.add_argument("--out", default=None, help="also write the section to this file")
    a = ap.parse_args()
    import meshfem_amd as M
    from meshfem_amd import grid
    from meshfem_amd._lib import ptr
    V, T = grid.grid_tet_mesh(a.n, a.n, a.n, [0, 0, 0], [1, 1, 1])
    c = M.Context(0)
    c.set_option("matrix_storage", 0)                  # both triangles from the start: the calls do not re-run the symbolic phase
    c.mesh_build(T, V, 2)
    c.material_isotropic(1.0, 0.3)
    c.set_preconditioner(M.PRECOND_MULTIGRID)
    sigma = np.zeros((c.n_elem, 6))
    sigma[:, 0] = -1.0
    c.set_prestress(sigma)
    n = c.bs * c.n_dof
    lines = ["## Measured: %d^3 grid, %d quadratic tets, %d unknowns" % (a.n, c.n_elem, n), ""]

    # (a) the assembly pass
    tl, tm, tg, td = (np.zeros(a.reps + 5) for _ in range(4))
    c._ck(c.lib.mfh_time_geometric_assembly(c.h, a.reps + 5, ptr(tl), ptr(tm), ptr(tg), ptr(td)))
    tl, tm, tg, td = tl[5:], tm[5:], tg[5:], td[5:]
    ml, mm, mg, md = (float(np.median(t)) for t in (tl, tm, tg, td))
    lines += ["Assembly pass into the one-double-per-block buffer, device events per launch, the flavours launched in turns, median of %d after 5"
              " warm-up rounds:" % a.reps, "",
              "| pass | ms (median) | min - max |", "|---|---|---|",
              "| MAT_LAPLACE (tr H) | %.3f | %.3f - %.3f |" % (ml, tl.min(), tl.max()),
              "| MAT_MASS (unit density) | %.3f | %.3f - %.3f |" % (mm, tm.min(), tm.max()),
              "| MAT_GEOM (H : sigma_e), plain flavour | %.3f | %.3f - %.3f |" % (mg, tg.min(), tg.max()),
              "| MAT_GEOM, turn-taking flavour (what ensure_geometric launches) | %.3f | %.3f - %.3f |" % (md, td.min(), td.max()), "",
              "ratio geometric / Laplacian: **%.3f**; geometric / unit mass: **%.3f**; turn-taking / plain geometric: **%.3f**" % (mg / ml, mg / mm, md / mg), ""]

    # (c) the per-call set-up of y = Kg x on the default storage
    if not a.no_apply:
        import time
        x = np.random.default_rng(1).standard_normal(n)
        y = np.empty_like(x)

        def timed(ctx, calls):
            out = []
            for _ in range(calls):
                t0 = time.perf_counter()
                ctx.geometric_apply(x, out=y)
                out.append((time.perf_counter() - t0) * 1e3)
            return out
        wide = timed(c, 4)
        d = M.Context(0)
        d.mesh_build(T, V, 2)
        d.material_isotropic(1.0, 0.3)
        d.set_prestress(sigma)
        dflt = timed(d, 3)
        d.close()
        lines += ["y = Kg x through the Python layer (host vectors of %d doubles up and down; host clock around the call):" % n, "",
                  "- option matrix_storage 0 (Kg assembled once): %s ms" % ", ".join("%.1f" % t for t in wide),
                  "- default options (upper-triangle storage: every call re-runs the symbolic phase with both triangles and reassembles Kg): %s ms" %
                  ", ".join("%.1f" % t for t in dflt), ""]

    # (b) the solve
    if not a.no_solve:
        c.bc_dirichlet_box([-1e-9, -1e9, -1e9], [1e-9, 1e9, 1e9], [0, 0, 0])
        fixed, _ = c.bc_dirichlet_vars()
        c.fix_variables(fixed)
        k_ms = c.time_spmv_kernel(reps=20)
        f = np.zeros(n)
        f[1::3] = -1.0
        c.solve(f, rtol=1e-6)                       # warm-up (hierarchy, lists)
        c.solve(f, rtol=1e-6)
        pcg_iter_ms = c.last_info["solve_ms"] / max(1, c.last_info["iterations"])
        cm = M.Context(0)
        cm.set_option("matrix_storage", 0)
        cm.mesh_build(T, V, 2)
        cm.set_operator(M.OP_MASS_VECTOR)
        cm.assemble()
        g_ms = cm.time_spmv_kernel(reps=20)
        cm.close()

        def run():
            try:
                return c.buckling(a.nev, rtol=a.rtol, maxit=a.maxit)
            except M.MeshFEMHipError:
                return c.last_buckling
        fac, X, info = run()                        # warm-up
        walls = []
        for _ in range(a.runs):
            fac, X, info = run()
            walls.append(info["solve_ms"])
        solve_ms = statistics.median(walls)
        its, m = info["iterations"], info["blockSize"]
        os.environ["MFH_MODES_TIMING"] = "1"
        (_, _, info_t), err = _capture_stderr(run)
        del os.environ["MFH_MODES_TIMING"]
        mt = re.search(r"ms: K ([\d.]+) M ([\d.]+) precond ([\d.]+) gram ([\d.]+) update ([\d.]+) residual ([\d.]+) rayleigh-ritz\(host\+sync\) ([\d.]+)", err)
        phases = [float(x) for x in mt.groups()] if mt else [float("nan")] * 7
        names = ["A products (Kg, k_spmv_kron)", "B products (K)", "preconditioner", "Gram (incl. download + synchronisation)", "block updates",
                 "residual kernel (incl. download)", "host Rayleigh-Ritz incl. its synchronisation"]
        lines += ["mfh_buckling, nev %d, multigrid, clamped on x = 0, sigma_xx = -1, rtol %g, maxit %d:" % (a.nev, a.rtol, a.maxit), "",
                  "- load factors: %s (converged %d, nBuckling %d)" % (np.array2string(fac, precision=6), info["converged"], info["nBuckling"]),
                  "- iterations %d, block size m = %d, restarts %d, locked at the end %d, max residual %.2e" %
                  (its, m, info["restarts"], info["nLocked"], info["maxResidual"]),
                  "- solve time (device events around the loop), %d runs after a warm-up: %s ms, median **%.1f ms** = %.2f ms per iteration; setup %.1f ms" %
                  (a.runs, ", ".join("%.1f" % w for w in walls), solve_ms, solve_ms / max(1, its), info["setup_ms"]),
                  "- note: %s" % (info["note"] or "(none)"), "",
                  "One further run with a stream synchronisation at every phase boundary (%.1f ms over %d iterations):" % (info_t["solve_ms"], info_t["iterations"]), "",
                  "| phase | ms per iteration | share |", "|---|---|---|"]
        tot = sum(phases)
        for nm, p in zip(names, phases):
            lines.append("| %s | %.3f | %.0f %% |" % (nm, p / max(1, info_t["iterations"]), 100 * p / tot if tot > 0 else 0))
        v_ms = max(pcg_iter_ms - k_ms, 0.0)
        floor = m * (k_ms + g_ms + v_ms)
        per_it = solve_ms / max(1, its)
        lines += ["",
                  "- K product (mfh_time_spmv_kernel, elasticity): %.3f ms" % k_ms,
                  "- Kg product (k_spmv_kron on the same pattern, timed as the MFH_OP_MASS_VECTOR product): %.3f ms" % g_ms,
                  "- one multigrid PCG iteration of mfh_solve on this context: %.3f ms, i.e. V-cycle + vector kernels = %.3f ms" % (pcg_iter_ms, v_ms),
                  "- floor per LOBPCG iteration with all m = %d columns active: m (K + Kg + V-cycle) = **%.2f ms**" % (m, floor),
                  "- measured per iteration: **%.2f ms**: %.2f x the floor" % (per_it, per_it / floor if floor > 0 else float("nan")), ""]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines))
    print("\n".join(lines))
    c.close()


if __name__ == "__main__":
    main()
