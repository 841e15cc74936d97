"""Record of prestressed vibration on one MI355X (docs/design/04_18_prestressed_modes.md) on BASELINE configs[2] (60^3 grid -> quadratic tets), clamped
on the face x = min under the uniform prestress sigma_xx = -1:
  (a) the pair product yA += s Kg x, yB = rho M x as ONE launch of k_spmv_kron_pair against the two launches (and the density scaling) it
      replaces, in alternating groups on the same context after a warm-up of both (mfh_time_kron_pair), repeated --rounds times: the spread;
  (b) mfh_buckling (nev 1) for the critical factor, then mfh_modes_prestressed at 0.5 of it against mfh_modes on the same context, nev 4,
      multigrid: iterations, time (device events around the loop) and the split by phase (one run each with a synchronisation at every phase
      boundary, MFH_MODES_TIMING);
  (c) the warm start: 0.55 of the critical factor cold, and started from the shapes at 0.5.
Prints the measured section of profiles/r14_prestressed_modes.md (and writes it to --out if given); the table of kernel resources in that file
comes from the compiler, not from this script."""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = r"ms: K ([\d.]+) M ([\d.]+) precond ([\d.]+) gram ([\d.]+) update ([\d.]+) residual ([\d.]+) rayleigh-ritz\(host\+sync\) ([\d.]+)"


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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=500)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--out", default=None, help="also write the section to this file")
    a = ap.parse_args()
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(a.n, a.n, a.n, [0, 0, 0], [1, 1, 1])
    c = M.Context(0)
    c.set_option("matrix_storage", 0)                  # both triangles from the start: the calls do not re-run the symbolic phase
    c.mesh_build(T, V, 2)
    c.material_isotropic(1.0, 0.3)
    c.set_preconditioner(M.PRECOND_MULTIGRID)
    sigma = np.zeros((c.n_elem, 6))
    sigma[:, 0] = -1.0
    c.set_prestress(sigma)
    c.bc_dirichlet_box([-1e-9, -1e9, -1e9], [1e-9, 1e9, 1e9], [0, 0, 0])
    fixed, _ = c.bc_dirichlet_vars()
    c.fix_variables(fixed)
    n = c.bs * c.n_dof
    lines = ["## Measured: %d^3 grid, %d quadratic tets, %d unknowns (%d fixed)" % (a.n, c.n_elem, n, len(fixed)), ""]

    # (a) the pair product
    pair, sep = [], []
    for _ in range(a.rounds):
        p, s = c.time_kron_pair(a.reps)
        pair.append(p)
        sep.append(s)
    mp, ms = statistics.median(pair), statistics.median(sep)
    lines += ["Pair product yA += s Kg x, yB = rho M x (rho = 1, the facades' default: the two-launch form pays no scaling kernel), device events around",
              "groups of %d launches, the two forms in alternating groups after a warm-up of both, %d rounds:" % (max(1, (a.reps + 3) // 4), a.rounds), "",
              "| form | ms per product (median of the rounds) | min - max |", "|---|---|---|",
              "| k_spmv_kron_pair, one launch | %.4f | %.4f - %.4f |" % (mp, min(pair), max(pair)),
              "| k_spmv_kron_acc + k_spmv_kron, two launches | %.4f | %.4f - %.4f |" % (ms, min(sep), max(sep)), "",
              "ratio single pass / separate launches: **%.3f**" % (mp / ms), ""]

    if not a.no_solve:
        k_ms = c.time_spmv_kernel(reps=20)

        def guarded(fn, last):
            try:
                return fn()
            except M.MeshFEMHipError:
                return getattr(c, last)
        cr = guarded(lambda: c.buckling(1, rtol=a.rtol, maxit=a.maxit), "last_buckling")[0][0]
        s5 = 0.5 * cr
        runs = {"mfh_modes": (lambda: c.modes(a.nev, rtol=a.rtol, maxit=a.maxit), "last_modes"),
                "mfh_modes_prestressed at 0.5 of the critical factor": (lambda: c.modes_prestressed(a.nev, s5, rtol=a.rtol, maxit=a.maxit), "last_modes_prestressed")}
        names = ["K products", "M products (prestressed: the pair product)", "preconditioner", "Gram (incl. download + synchronisation)", "block updates",
                 "residual kernel (incl. download)", "host Rayleigh-Ritz incl. its synchronisation"]
        lines += ["Critical factor of the prestress (mfh_buckling, nev 1): %.6g. K product (mfh_time_spmv_kernel): %.3f ms." % (cr, k_ms), ""]
        table = {}
        shapes = None
        for tag, (fn, last) in runs.items():
            guarded(fn, last)                          # warm-up
            walls = []
            for _ in range(a.runs):
                lam, X, info = guarded(fn, last)
                walls.append(info["solve_ms"])
            if "prestressed" in tag:
                shapes = X
            solve_ms = statistics.median(walls)
            its = max(1, info["iterations"])
            os.environ["MFH_MODES_TIMING"] = "1"
            (_, _, info_t), err = _capture_stderr(lambda: guarded(fn, last))
            del os.environ["MFH_MODES_TIMING"]
            mt = re.search(PHASES, err)
            table[tag] = ([float(x) / max(1, info_t["iterations"]) for x in mt.groups()] if mt else [float("nan")] * 7, info_t["iterations"])
            lines += ["%s, nev %d, multigrid, rtol %g:" % (tag, a.nev, a.rtol), "",
                      "- lambda: %s (converged %d)" % (np.array2string(lam, precision=6), info["converged"]),
                      "- iterations %d, block size m = %d, restarts %d, max residual %.2e" % (info["iterations"], info["blockSize"], info["restarts"], info["maxResidual"]),
                      "- solve time (device events around the loop), %d runs after a warm-up: %s ms, median **%.1f ms** = %.2f ms per iteration; setup %.1f ms" %
                      (a.runs, ", ".join("%.1f" % w for w in walls), solve_ms, solve_ms / its, info["setup_ms"]),
                      "- note: %s" % (info["note"] or "(none)"), ""]
        tags = list(runs)
        lines += ["One further run each with a stream synchronisation at every phase boundary, ms per iteration (%d and %d iterations):" %
                  (table[tags[0]][1], table[tags[1]][1]), "", "| phase | mfh_modes | mfh_modes_prestressed |", "|---|---|---|"]
        for i, nm in enumerate(names):
            lines.append("| %s | %.3f | %.3f |" % (nm, table[tags[0]][0][i], table[tags[1]][0][i]))
        lines += ["| sum | %.3f | %.3f |" % (sum(table[tags[0]][0]), sum(table[tags[1]][0])), ""]

        # (c) the warm start
        s55 = 0.55 * cr
        _, _, cold = guarded(lambda: c.modes_prestressed(a.nev, s55, rtol=a.rtol, maxit=a.maxit), "last_modes_prestressed")
        _, _, warm = guarded(lambda: c.modes_prestressed(a.nev, s55, x0=shapes, rtol=a.rtol, maxit=a.maxit), "last_modes_prestressed")
        lines += ["Warm start at 0.55 of the critical factor: %d iterations, %.1f ms cold; %d iterations, %.1f ms started from the shapes at 0.5." %
                  (cold["iterations"], cold["solve_ms"], warm["iterations"], warm["solve_ms"]), ""]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines))
    print("\n".join(lines))
    c.close()


if __name__ == "__main__":
    main()
