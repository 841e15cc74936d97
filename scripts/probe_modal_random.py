"""Record of the random-vibration layer on one MI355X: the setup of scripts/probe_modal.py (BASELINE configs[2], 60^3 quadratic tets, clamped on the face
x = 0, 64 modes by mfh_modes_many, 2 % modal damping), one load. Writes profiles/r20_modal_random.md (or --out):
  - one pass of k_modal_sumsq<32> against one pass of k_modal_expand<32> on the same hashed columns (mfh_time_modal_sumsq), the two taking turns,
    --rounds rounds in this process, each against its byte floor
  - whole modal_random calls at 1 000 and 10 000 grid points with the static correction: covariance (host), factorisation (host), passes (device)
  - the caller's alternative without this layer: modal_harmonic fields of --alt-freqs frequencies summed on the host, scaled by count (stated as scaled)
  - set_modal_basis_from_modes after modes_many (the handover on the device) against set_modal_basis of the host copy
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--alt-freqs", type=int, default=64)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--maxit", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r20_modal_random.md"))
    a = ap.parse_args()
    import meshfem_amd as M
    from meshfem_amd import grid
    lines = ["# Random vibration on one MI355X: %d^3 quadratic tets, clamped on x = 0, %d modes, 2 %% modal damping" % (a.n, a.modes), ""]

    def say(*ls):
        lines.extend(ls)
        print("\n".join(ls), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    V, T = grid.grid_tet_mesh(a.n, a.n, a.n, [0, 0, 0], [1, 1, 1])
    c = M.Context(0)
    c.set_option("matrix_storage", 0)
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

    # ---- one pass of either kernel
    nb = a.modes + 2
    say("## One pass: k_modal_sumsq<32> against k_modal_expand<32>, %d columns of %d rows" % (nb, n), "",
        "%d rounds in this process; in each the two take turns, 3 launches each (one event pair per launch). Median [min, max] in ms." % a.rounds,
        "Byte floors: sumsq reads nb columns, reads nothing else on a first pass and writes one plane -- (nb + 1) n 8 B here, (nb + 2) n 8 B on a later",
        "pass that reads the accumulator back; expand reads nb columns and writes 32 planes, (nb + 32) n 8 B. Floors at 8 TB/s.", "",
        "| kernel | ms | byte floor ms | ms / floor |", "|---|---|---|---|")
    s, e, l = [], [], []
    for _ in range(a.rounds):
        ts, te, tl = c.time_modal_sumsq(n, nb, 32, reps=3)
        s.extend(ts)
        e.extend(te)
        l.extend(tl)
    s, e, l = np.array(s), np.array(e), np.array(l)
    fl_s, fl_e, fl_l = (nb + 1) * n * 8 / 8e12 * 1e3, (nb + 32) * n * 8 / 8e12 * 1e3, (nb - 32 + 2) * n * 8 / 8e12 * 1e3
    say("| k_modal_sumsq<32> | %.3f [%.3f, %.3f] | %.3f | %.2f |" % (np.median(s), s.min(), s.max(), fl_s, np.median(s) / fl_s),
        "| k_modal_sumsq<32>, second pass of a rank-64 factor: nc = %d columns, (nc + 2) n 8 B | %.3f [%.3f, %.3f] | %.3f | %.2f |" % (nb - 32, np.median(l), l.min(), l.max(), fl_l, np.median(l) / fl_l),
        "| k_modal_expand<32> | %.3f [%.3f, %.3f] | %.3f | %.2f |" % (np.median(e), e.min(), e.max(), fl_e, np.median(e) / fl_e), "",
        "Acceptance: the sum-of-squares pass is %s than the expansion pass beyond the latter's run-to-run range (%.3f ms) in this run." %
        ("not slower" if np.median(s) <= np.median(e) + (e.max() - e.min()) else "SLOWER", e.max() - e.min()), "")

    # ---- the basis: the handover on the device against the host round trip
    t0 = time.time()
    lam, X, info = c.modes_many(a.modes, batch=16, rtol=1e-6, maxit=3000)
    t_modes = time.time() - t0
    t0 = time.time()
    ai = c.set_modal_basis_from_modes(a.modes)
    t_adopt = time.time() - t0
    t0 = time.time()
    bi = c.set_modal_basis(lam, X)
    t_set = time.time() - t0
    c.set_modal_basis_from_modes(a.modes)          # (the basis of what follows: the adopted one)
    gb = X.nbytes / 1e9
    del X
    say("## The basis", "", "modes_many(%d): %.1f s wall (it returns %.1f GB to the host and keeps its set on the device)." % (a.modes, t_modes, gb),
        "set_modal_basis_from_modes: %.3f s wall, %.0f ms by device events (%d signed column copies on the device, %d mass products, the Gram kernel); orthoDefect %.2e."
        % (t_adopt, ai["setupMs"], a.modes, a.modes, ai["orthoDefect"]),
        "set_modal_basis of the host copy (the round trip's second half): %.3f s wall, %.0f ms by device events (the upload of those %.1f GB instead of the copies); orthoDefect %.2e."
        % (t_set, bi["setupMs"], gb, bi["orthoDefect"]), "")
    w = np.sqrt(lam)

    # ---- whole calls
    say("## modal_random, static correction, sigma_u field and two probes", "",
        "| grid points | wall s | covarianceMs (host) | factorMs (host) | passes and the copy of the plane(s) to the host, ms by device events | rank | passes | truncation | static iterations |", "|---|---|---|---|---|---|---|---|---|")
    probes = [n - 2, n // 2]
    for nf in (1000, 10000):
        om = np.linspace(0.2 * w[0], 1.1 * w[-1], nf)
        S = 1.0 / (1.0 + (om / w[0]) ** 2)
        c.modal_random(om[:50], S[:50], f, modal_damping=0.02, rtol=a.rtol, maxit=a.maxit, probes=probes)          # warm-up
        t0 = time.time()
        r = c.modal_random(om, S, f, modal_damping=0.02, rtol=a.rtol, maxit=a.maxit, probes=probes)
        wall = time.time() - t0
        i = r["info"]
        say("| %d | %.3f | %.1f | %.2f | %.2f | %d | %d | %.2e | %d |" % (nf, wall, i["covarianceMs"], i["factorMs"], i["solveMs"], i["ranks"][0], i["passes"][0], i["truncation"][0],
                                                                    i["staticIterations"]))
    say("", "(wall includes the static solve, the load projection and the copy of one plane to the host.)", "")
    t0 = time.time()
    r3 = c.modal_random(om, S, f, modal_damping=0.02, rtol=a.rtol, maxit=a.maxit, probes=probes, velocity=True, acceleration=True)
    i = r3["info"]
    say("With sigma_v and sigma_a as well (10 000 points): wall %.3f s, passes and copies %.2f ms, ranks %s." % (time.time() - t0, i["solveMs"], i["ranks"]), "")

    # ---- the caller's alternative
    k = a.alt_freqs
    c.modal_harmonic(om[:2], f, modal_damping=0.02, rtol=a.rtol, maxit=a.maxit)                                       # warm-up
    t0 = time.time()
    h = c.modal_harmonic(om[:k], f, modal_damping=0.02, rtol=a.rtol, maxit=a.maxit)
    t_h = time.time() - t0
    t1 = time.time()
    acc = ((S[:k, None]) * (h["u"].real ** 2 + h["u"].imag ** 2)).sum(axis=0)
    t_sum = time.time() - t1
    say("## The caller's alternative: summing modal_harmonic fields", "",
        "%d frequencies: modal_harmonic %.2f s wall (solveMs %.0f on the device, the rest the copy of %.1f GB to the host), the weighted sum of squares in numpy %.2f s."
        % (k, t_h, h["info"]["solveMs"], h["u"].nbytes / 1e9, t_sum),
        "SCALED by count, not measured: %.0f s for 1 000 grid points, %.0f s for 10 000." % ((t_h + t_sum) * 1000 / k, (t_h + t_sum) * 10000 / k), "")
    del h, acc
    c.close()


if __name__ == "__main__":
    main()
