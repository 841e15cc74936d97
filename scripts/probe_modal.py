"""Record of modal superposition on one MI355X: BASELINE configs[2] (60^3 quadratic tets) clamped on the face x = 0, the Rayleigh case of
scripts/probe_harmonic.py (0.1 omega_1, 0.02 / omega_1), 64 modes by mfh_modes_many, 1 000 frequencies in [0.5, 3] omega_1. Writes
profiles/r18_modal.md (or --out):
  - the time of modes_many and of set_modal_basis
  - ms per pass of k_modal_expand<NP> for NP in {8, 16, 32} at nb = 64 beside its byte floor (nb + NP) n 8 B / 6.29 TB/s and beside
    k_deflate_update<16> on the same shape, the variants taking turns inside this process, several rounds (median and range)
  - the sweep's time with probes only (1 000 frequencies) and with fields (--field-freqs frequencies: a field row is 357 MB on the host)
  - the cost per frequency beside mfh_harmonic's on the same context at omega in {0.5, 1.5, 3} omega_1
  - the true residuals and the difference from mfh_harmonic's u^ at those three frequencies, with and without static correction
Every timed call is preceded by a warm-up call of the same shape."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12      # B/s, the device-to-device copy rate of the MI355X the byte floors are stated against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60, help="grid cells per axis (BASELINE configs[2]: 60)")
    ap.add_argument("--modes", type=int, default=64)
    ap.add_argument("--freqs", type=int, default=1000)
    ap.add_argument("--field-freqs", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--maxit", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r18_modal.md"))
    a = ap.parse_args()
    import meshfem_amd as M
    from meshfem_amd import grid
    lines = ["# Modal superposition on one MI355X: %d^3 quadratic tets, clamped on x = 0, %d modes, Rayleigh damping (0.1 omega_1, 0.02 / omega_1)" % (a.n, a.modes), ""]

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

    # ---- the kernel, before the basis takes its memory
    nb = 64
    t = {8: [], 16: [], 32: [], "deflate": [], "copy": []}
    for _ in range(a.rounds):
        for NP in (8, 16, 32):
            t[NP].extend(c.time_modal_expand(n, nb, NP, reps=3))
        _, upd, cp = c.time_deflate(n, nb, 16, reps=3)
        t["deflate"].append(upd)
        t["copy"].append(cp)
    say("## k_modal_expand<NP>, one pass at nb = %d columns of %d rows" % (nb, n), "",
        "%d rounds; in each the three instantiations (3 launches each, one event pair per launch) and mfh_time_deflate (k_deflate_update<16> on %d + 16" % (a.rounds, nb),
        "columns, 3 launches per event pair, and a device-to-device copy of the same %d columns) take turns. Median [min, max] in ms. Floor: (nb + NP) n 8 B at" % (nb + 16),
        "6.29 TB/s. One lane per row; a variant with two adjacent rows per lane (16-byte loads) was not built.", "",
        "| kernel | ms per pass | floor ms | pass / floor | ms per plane |", "|---|---|---|---|---|")
    for NP in (8, 16, 32):
        v = np.array(t[NP])
        floor = (nb + NP) * n * 8 / COPY_RATE * 1e3
        say("| k_modal_expand<%d> | %.3f [%.3f, %.3f] | %.3f | %.2f | %.3f |" % (NP, np.median(v), v.min(), v.max(), floor, np.median(v) / floor, np.median(v) / NP))
    v, cp = np.array(t["deflate"]), np.array(t["copy"])
    floor = (nb + 2 * 16) * n * 8 / COPY_RATE * 1e3
    say("| k_deflate_update<16> (reads and writes its 16 columns) | %.3f [%.3f, %.3f] | %.3f | %.2f | - |" % (np.median(v), v.min(), v.max(), floor, np.median(v) / floor),
        "| device-to-device copy of %d columns | %.3f [%.3f, %.3f] | - | - | - |" % (nb + 16, np.median(cp), cp.min(), cp.max()), "")
    e16 = np.array(t[16])
    spread = v.max() - v.min()
    say("Acceptance: k_modal_expand<16> %.3f ms against k_deflate_update<16> %.3f ms (its own run-to-run range %.3f ms): %s." %
        (np.median(e16), np.median(v), spread, "not slower" if np.median(e16) <= np.median(v) + spread else "SLOWER"), "")

    # ---- the basis
    t0 = time.time()
    lam, X, info = c.modes_many(a.modes, batch=16, rtol=1e-6, maxit=3000)
    t_modes = time.time() - t0
    w1 = float(np.sqrt(lam[0]))
    t0 = time.time()
    bi = c.set_modal_basis(lam, X)
    t_set = time.time() - t0
    say("## The basis", "",
        "- modes_many(%d): %.1f s wall (solve %.0f ms, setup %.0f ms by device events), %d iterations in %d batches; omega_1 = %.6g, omega_%d = %.6g" %
        (a.modes, t_modes, info["solve_ms"], info["setup_ms"], info["iterations"], info["batches"], w1, a.modes, float(np.sqrt(lam[-1]))),
        "- set_modal_basis: %.2f s wall (%.0f ms by device events: the upload of %.1f GB, %d mass products, the Gram kernel), %.2f GB on the device, orthoDefect %.2e" %
        (t_set, bi["setupMs"], X.nbytes / 1e9, a.modes, bi["deviceBytes"] / 1e9, bi["orthoDefect"]), "")
    del X
    damping = (0.1 * w1, 0.02 / w1)
    om = np.linspace(0.5, 3.0, a.freqs) * w1
    om3 = np.array([0.5, 1.5, 3.0]) * w1
    probes = [n - 2, n // 2]

    # ---- the sweep
    say("## The sweep", "", "| run | frequencies | wall s | setupMs (load, Gram, static solve) | solveMs | ms per frequency | groups |", "|---|---|---|---|---|---|---|")
    for name, kw, freqs in (("probes only, static correction", dict(fields=False, probes=probes), om),
                            ("probes only, no correction", dict(fields=False, probes=probes, static_correction=False), om),
                            ("fields + probes, static correction", dict(fields=True, probes=probes), om[:: max(1, a.freqs // a.field_freqs)][: a.field_freqs])):
        c.modal_harmonic(freqs[:2], f, damping=damping, rtol=a.rtol, maxit=a.maxit, **kw)            # warm-up
        t0 = time.time()
        r = c.modal_harmonic(freqs, f, damping=damping, rtol=a.rtol, maxit=a.maxit, **kw)
        wall = time.time() - t0
        i = r["info"]
        say("| %s | %d | %.3f | %.1f | %.1f | %.4f | %d |" % (name, len(freqs), wall, i["setupMs"], i["solveMs"], i["solveMs"] / len(freqs), i["groups"]))
        del r
    say("")

    # ---- beside mfh_harmonic
    c.harmonic(om3[:1], f, damping=damping, rtol=1e-3, maxit=a.maxit, fields=False)                  # warm-up
    t0 = time.time()
    h = c.harmonic(om3, f, damping=damping, rtol=a.rtol, maxit=a.maxit, warm_start=False)
    t_h = time.time() - t0
    say("## Beside mfh_harmonic (rtol %g, cold starts) at omega in {0.5, 1.5, 3} omega_1" % a.rtol, "",
        "mfh_harmonic: %.2f s wall, solveMs %.0f for %d iterations: %.0f ms per frequency." % (t_h, h["info"]["solveMs"], h["info"]["iterationsTotal"], h["info"]["solveMs"] / 3), "",
        "| omega / omega_1 | COCG iterations | static correction | true residual of the modal u^ | ||u^_modal - u^_harmonic|| / ||u^_harmonic|| |", "|---|---|---|---|---|")
    for corrected in (True, False):
        r = c.modal_harmonic(om3, f, damping=damping, rtol=a.rtol, maxit=a.maxit, static_correction=corrected, residual_stride=0)
        for k in range(3):
            d = np.linalg.norm(r["u"][k] - h["u"][k]) / np.linalg.norm(h["u"][k])
            say("| %.1f | %d | %s | %.3e | %.3e |" % (om3[k] / w1, h["iterations"][k], "yes" if corrected else "no", r["true_residuals"][k], d))
        del r
    say("")
    c.close()


if __name__ == "__main__":
    main()
