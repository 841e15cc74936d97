"""Record of the vibrational-mode solver on one MI355X: BASELINE configs[2] (60^3 quadratic tets) clamped on the face x = min, nev = 8, multigrid.
Writes profiles/r08_modes.md (or --out): iteration count, time per iteration split by phase (one run with a synchronisation at every phase
boundary, MFH_MODES_TIMING), the whole call without those synchronisations (median of --runs after a warm-up), k_block_gram against a
device-to-device copy of the same bytes in this process, and the floor the call cannot beat -- m K-products + m M-products + m
preconditioner applications per iteration -- from mfh_time_spmv_kernel and the timers of a PCG solve on the same context."""
import argparse
import os
import re
import statistics
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60, help="grid cells per axis (BASELINE configs[2]: 60)")
    ap.add_argument("--nev", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r08_modes.md"))
    a = ap.parse_args()
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(a.n, a.n, a.n, [0, 0, 0], [1, 1, 1])
    c = M.Context(0)
    c.set_option("matrix_storage", 0)          # both triangles from the start: the call does not re-run the symbolic phase
    c.mesh_build(T, V, 2)
    c.material_isotropic(1.0, 0.3)
    c.set_preconditioner(M.PRECOND_MULTIGRID)
    c.bc_dirichlet_box([-1e-9, -1e9, -1e9], [1e-9, 1e9, 1e9], [0, 0, 0])
    fixed, _ = c.bc_dirichlet_vars()
    c.fix_variables(fixed)
    n = c.bs * c.n_dof
    lines = ["# Vibrational modes on one MI355X: %d^3 quadratic tets, clamped on x = 0, nev = %d, multigrid, rtol %g" % (a.n, a.nev, a.rtol), "",
             "%d elements, %d unknowns (%d fixed)." % (c.n_elem, n, len(fixed)), ""]
    # ---- the floor: the parent commit's kernels
    k_ms = c.time_spmv_kernel(reps=20)
    f = np.zeros(n); f[1::3] = -1.0
    c.solve(f, rtol=1e-6)                       # warm-up (hierarchy, lists)
    c.solve(f, rtol=1e-6)
    pcg_iter_ms = c.last_info["solve_ms"] / max(1, c.last_info["iterations"])
    cm = M.Context(0)
    cm.set_option("matrix_storage", 0)
    cm.mesh_build(T, V, 2)
    cm.set_operator(M.OP_MASS_VECTOR)
    cm.assemble()
    m_ms = cm.time_spmv_kernel(reps=20)
    cm.close()
    # ---- the call
    lam, X, info = c.modes(a.nev, rtol=a.rtol, maxit=500)        # warm-up
    walls = []
    for _ in range(a.runs):
        lam, X, info = c.modes(a.nev, rtol=a.rtol, maxit=500)
        walls.append(info["solve_ms"])
    solve_ms = statistics.median(walls)
    its, m = info["iterations"], info["blockSize"]
    os.environ["MFH_MODES_TIMING"] = "1"
    (_, _, info_t), err = _capture_stderr(lambda: c.modes(a.nev, rtol=a.rtol, maxit=500))
    del os.environ["MFH_MODES_TIMING"]
    mt = re.search(r"ms: K ([\d.]+) M ([\d.]+) precond ([\d.]+) gram ([\d.]+) update ([\d.]+) residual ([\d.]+) rayleigh-ritz\(host\+sync\) ([\d.]+)", err)
    phases = [float(x) for x in mt.groups()] if mt else [float("nan")] * 7
    names = ["K products", "M products", "preconditioner", "Gram (incl. download + synchronisation)", "block updates", "residual kernel (incl. download)",
             "host Rayleigh-Ritz incl. its synchronisation"]
    lines += ["## The call", "",
              "- lambda: %s" % np.array2string(lam, precision=6),
              "- iterations %d, block size m = %d, restarts %d, locked at the end %d, max residual %.2e" % (its, m, info["restarts"], info["nLocked"], info["maxResidual"]),
              "- solve time (device events around the loop), %d runs after a warm-up: %s ms, median **%.1f ms** = %.2f ms per iteration; setup %.1f ms" %
              (a.runs, ", ".join("%.1f" % w for w in walls), solve_ms, solve_ms / max(1, its), info["setup_ms"]),
              "- note: %s" % (info["note"] or "(none)"), "",
              "## Time per iteration by phase", "",
              "One further run with a stream synchronisation at every phase boundary (so the phases add up to more than the free-running call: %.1f ms over %d iterations)." %
              (info_t["solve_ms"], info_t["iterations"]), "",
              "| phase | ms per iteration | share |", "|---|---|---|"]
    tot = sum(phases)
    for nm, p in zip(names, phases):
        lines.append("| %s | %.3f | %.0f %% |" % (nm, p / max(1, info_t["iterations"]), 100 * p / tot if tot > 0 else 0))
    # ---- Gram kernel against a copy
    lines += ["", "## k_block_gram against a device-to-device copy of the same bytes (same process)", "",
              "The kernel reads n (p + q) doubles once; the copy reads AND writes them.", "",
              "| p x q | bytes read | gram ms | GB/s read | copy ms | gram / copy |", "|---|---|---|---|---|---|"]
    for p, q in ((m, m), (24, 24), (6, 8)):
        g_ms, cp_ms = c.time_block_gram(n, p, q, reps=10)
        by = 8.0 * n * (p + q)
        lines.append("| %d x %d | %.0f MB | %.3f | %.0f | %.3f | %.2f |" % (p, q, by / 1e6, g_ms, by / g_ms / 1e6, cp_ms, g_ms / cp_ms))
    lines += ["", "Only the VALU-tile variant of the Gram kernel is built; an FP64 MFMA (16x16x4) variant was not built and is not measured.", ""]
    # ---- the floor
    v_ms = max(pcg_iter_ms - k_ms, 0.0)
    floor = m * (k_ms + m_ms + v_ms)
    per_it = solve_ms / max(1, its)
    lines += ["## The floor", "",
              "- K product (mfh_time_spmv_kernel, elasticity, matrix-free): %.3f ms" % k_ms,
              "- M product (mfh_time_spmv_kernel, MFH_OP_MASS_VECTOR, k_spmv_kron): %.3f ms" % m_ms,
              "- one multigrid PCG iteration of mfh_solve on this context: %.3f ms, i.e. V-cycle + vector kernels = %.3f ms" % (pcg_iter_ms, v_ms),
              "- floor per LOBPCG iteration with all m = %d columns active: m (K + M + V-cycle) = **%.2f ms**" % (m, floor),
              "- measured per iteration: **%.2f ms**: %.2f x the floor (converged columns are locked, so late iterations apply fewer than m operators;"
              " the block kernels and the host step are what is above m_active x the operator cost)" % (per_it, per_it / floor if floor > 0 else float("nan")), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))
    c.close()


if __name__ == "__main__":
    main()
