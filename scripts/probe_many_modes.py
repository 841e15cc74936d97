"""Record of mfh_modes_many on one MI355X (docs/design/04_19_many_modes.md) on BASELINE configs[2] (60^3 grid -> quadratic tets), clamped on the
face x = min, multigrid:
  (a) k_deflate_gram (+ its second stage) and k_deflate_update against a device-to-device copy of the same nq + k columns in the same process
      (mfh_time_deflate), at the row count of the mesh, for the full set (256 x 24) and for what a 64-mode run sees (16 .. 48 x 20, and 8 active);
  (b) 64 modes in batches of 16, with the guard columns of a batch seeding the next start block and without (env MFH_MODES_MANY_NO_SEED):
      iterations and device time per batch (the library's own per-batch line, env MFH_MODES_MANY_LOG), the full residuals;
  (c) one further seeded run with a synchronisation at every phase boundary (MFH_MODES_TIMING): the share of the deflation kernels.
Prints the measured section of profiles/r15_many_modes.md (and writes it to --out if given); the table of kernel resources in that file comes
from the compiler, not from this script."""
import argparse
import datetime
import os
import re
import socket
import sys
import tempfile


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = (r"iterations (\d+) \| ms: K ([\d.]+) M ([\d.]+) precond ([\d.]+) gram ([\d.]+) update ([\d.]+) residual ([\d.]+) "
          r"rayleigh-ritz\(host\+sync\) ([\d.]+) deflation ([\d.]+)")
BATCH = r"batch (\d+): (\d+) modes, set (\d+), seeded (\d+), iterations (\d+), setup ([\d.]+) ms, solve ([\d.]+) ms"


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
    ap.add_argument("--nev", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
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
    c.bc_dirichlet_box([-1e-9, -1e9, -1e9], [1e-9, 1e9, 1e9], [0, 0, 0])
    fixed, _ = c.bc_dirichlet_vars()
    c.fix_variables(fixed)
    n = c.bs * c.n_dof
    lines = ["## Measured: %d^3 grid, %d quadratic tets, %d unknowns (%d fixed)" % (a.n, c.n_elem, n, len(fixed)), "",
             "Host %s, %s." % (socket.gethostname(), datetime.date.today().isoformat()), ""]

    # (a) the kernels against a copy of the same columns
    lines += ["Projection kernels at %d rows, ms per call (device events around %d calls after a warm-up), against a device-to-device copy of the" % (n, a.reps),
              "same nq + k columns in the same process (a copy reads and writes every byte; the Gram kernel only reads, the update reads all and",
              "writes k columns):", "", "| nq | k | columns read by the Gram kernel | k_deflate_gram | k_deflate_update | copy | gram / copy | update / copy |",
              "|---|---|---|---|---|---|---|---|"]
    for nq, k in ((256, 24), (256, 8), (48, 20), (16, 20), (48, 8)):
        g, u, cp = c.time_deflate(n, nq, k, a.reps)
        qg = 6 * (12 // ((k + 7) // 8))
        reads = nq + k * ((nq + qg - 1) // qg)
        lines.append("| %d | %d | %d (minimum %d) | %.3f | %.3f | %.3f | %.2f | %.2f |" % (nq, k, reads, nq + k, g, u, cp, g / cp, u / cp))
    lines.append("")
    print("[probe] kernels timed", flush=True)

    if not a.no_solve:
        def guarded(fn):
            try:
                return fn()
            except M.MeshFEMHipError:
                return c.last_modes_many

        def run():
            return guarded(lambda: c.modes_many(a.nev, batch=a.batch, rtol=a.rtol, maxit=a.maxit))
        os.environ["MFH_MODES_MANY_LOG"] = "1"
        table = {}
        for tag, env in (("guard columns seed the next batch", None), ("every batch starts from the hashed block", "MFH_MODES_MANY_NO_SEED")):
            if env:
                os.environ[env] = "1"
            (lam, X, info), err = _capture_stderr(run)
            if env:
                del os.environ[env]
            rows = [tuple(float(x) for x in m) for m in re.findall(BATCH, err)]
            table[tag] = (rows, info)
            print("[probe] run done: %s" % tag, flush=True)
            lines += ["%d modes in batches of %d, multigrid, rtol %g, lockFactor 0.1 -- %s:" % (a.nev, a.batch, a.rtol, tag), "",
                      "- converged %d, %d batches, %d iterations in all, restarts %d, out of order %d" %
                      (info["converged"], info["batches"], info["iterations"], info["restarts"], info["nOutOfOrder"]),
                      "- largest full residual %.3e = %.3f rtol; largest |Q^T M x| before the last projection of a batch %.2e" %
                      (info["maxResidual"], info["maxResidual"] / a.rtol, info["maxLockDefect"]),
                      "- lambda[0] %.6g, lambda[%d] %.6g" % (lam[0], len(lam) - 1, lam[-1]),
                      "- solve %.1f ms, setup %.1f ms (device events)" % (info["solve_ms"], info["setup_ms"]), "",
                      "| batch | modes | columns in the set | seeded columns | iterations | setup ms | solve ms | ms per iteration |", "|---|---|---|---|---|---|---|---|"]
            for r in rows:
                lines.append("| %d | %d | %d | %d | %d | %.1f | %.1f | %.1f |" % (r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[6] / max(1.0, r[4])))
            lines.append("")
        tags = list(table)
        it_seed, it_cold = (sum(r[4] for r in table[t][0][1:]) for t in tags)
        lines += ["Iterations of the batches after the first: %d seeded, %d from the hashed block: the seeding saves %d (%.0f %%)." %
                  (it_seed, it_cold, it_cold - it_seed, 100.0 * (it_cold - it_seed) / max(1.0, it_cold)), ""]
        del os.environ["MFH_MODES_MANY_LOG"]

        # (c) the share of the deflation kernels
        os.environ["MFH_MODES_TIMING"] = "1"
        (_, _, info_t), err = _capture_stderr(run)
        del os.environ["MFH_MODES_TIMING"]
        found = re.findall(PHASES, err)
        if found:
            its = info_t["iterations"]
            ph = [float(x) for x in found[-1][1:]]         # the record accumulates over the batches: the last line holds the whole call
            names = ["K products", "M products", "preconditioner", "Gram (incl. download + synchronisation)", "block updates", "residual kernel (incl. download)",
                     "host Rayleigh-Ritz incl. its synchronisation", "deflation: k_deflate_gram, the coefficients' host trip, k_deflate_update"]
            lines += ["One further seeded run with a stream synchronisation at every phase boundary (%d iterations in all):" % its, "",
                      "| phase | ms in all | ms per iteration | share |", "|---|---|---|---|"]
            for nm, v in zip(names, ph):
                lines.append("| %s | %.1f | %.3f | %.1f %% |" % (nm, v, v / max(1, its), 100.0 * v / sum(ph)))
            lines += ["| sum | %.1f | %.3f | |" % (sum(ph), sum(ph) / max(1, its)), ""]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines))
    print("\n".join(lines))
    c.close()


if __name__ == "__main__":
    main()
