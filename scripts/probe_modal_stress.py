"""Record of the modal stress recovery on one MI355X: the setup of scripts/probe_modal_random.py (BASELINE configs[2], 60^3 quadratic tets, clamped on
the face x = 0, 64 modes by mfh_modes_many, 2 % modal damping), one load. Writes profiles/r21_modal_stress.md (or --out):
  - one pass of k_modal_stress_sumsq over 32 hashed planes against 32 launches of k_stress_measures (von Mises only) on the same planes
    (mfh_time_modal_stress), the two taking turns, --rounds rounds in this process; the new kernel against its byte floor
  - the expansion pass beside it (mfh_time_modal_expand: nb columns into 32 planes)
  - a whole modal_random_stress at 1 000 grid points with the static correction: covariance (host), factorisation (host), passes (device)
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
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--maxit", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r21_modal_stress.md"))
    a = ap.parse_args()
    import meshfem_amd as M
    from meshfem_amd import grid
    lines = ["# Modal stress recovery on one MI355X: %d^3 quadratic tets, clamped on x = 0, %d modes, 2 %% modal damping" % (a.n, a.modes), ""]

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
    ne = c.n_elem
    f = np.zeros(n)
    f[1::3] = -1.0 / n
    c.solve(f, rtol=1e-6)                       # warm-up (hierarchy, lists)
    say("%d elements, %d unknowns (%d fixed)." % (ne, n, len(fixed)), "")

    # ---- one pass of the new kernel against 32 launches of the existing one
    NP, NPE, NQ, GEO = 32, 10, 4, 16          # GEO: GEO_ISO_STRIDE of mfh_internal.hh, assumed (the generated text says so)
    planes_b, nodes_b, geo_b, out_b = NP * n * 8, ne * NPE * 4, ne * GEO * 8, ne * NQ * 8
    floor = (planes_b + nodes_b + geo_b + out_b) / 8e12 * 1e3
    gathered = NP * ne * NPE * 3 * 8
    say("## One pass: k_modal_stress_sumsq over %d planes against %d launches of k_stress_measures" % (NP, NP), "",
        "%d rounds in this process; in each the two take turns, 3 repetitions each (one event pair per repetition). Median [min, max] in ms." % a.rounds,
        "Both write the von Mises value only (isotropic material, stress). Byte floor of the new kernel: the planes read once + the element records",
        "(node list 10 x 4 B, geometry and material %d x 8 B per element) + the output, (%d n 8 + nElem (40 + %d + 32)) B = %.2f GB, at 8 TB/s." %
        (GEO, NP, GEO * 8, (planes_b + nodes_b + geo_b + out_b) / 1e9),
        "The gather asks for 32 x nElem x 10 nodes x 3 x 8 B = %.2f GB of nodal values, %.1f x the planes themselves (every node is shared by several" %
        (gathered / 1e9, gathered / planes_b),
        "elements); how much of that comes from the caches and how much from memory is not measured here (a counter run would say).",
        "Assumed, not read from the library: the 16 doubles (one 128 B line) of an isotropic element record (GEO_ISO_STRIDE, mfh_internal.hh) and 8 TB/s of",
        "memory bandwidth; the \"ms / floor\" column stands on both.", "",
        "| | ms | per plane ms | byte floor ms | ms / floor |", "|---|---|---|---|---|")
    s, m = [], []
    for _ in range(a.rounds):
        ts, tm = c.time_modal_stress(NP, reps=3)
        s.extend(ts)
        m.extend(tm)
    s, m = np.array(s), np.array(m)
    say("| k_modal_stress_sumsq, one pass of %d planes | %.3f [%.3f, %.3f] | %.4f | %.3f | %.2f |" % (NP, np.median(s), s.min(), s.max(), np.median(s) / NP, floor, np.median(s) / floor),
        "| k_stress_measures, %d launches | %.3f [%.3f, %.3f] | %.4f | | |" % (NP, np.median(m), m.min(), m.max(), np.median(m) / NP), "",
        "New kernel per plane / k_stress_measures per plane: %.3f (medians); ranges of the two: %.3f ms and %.3f ms." %
        (np.median(s) / np.median(m), s.max() - s.min(), m.max() - m.min()), "")

    # ---- the expansion pass beside it
    nb = a.modes + 2
    e = []
    for _ in range(a.rounds):
        e.extend(c.time_modal_expand(n, nb, 32, reps=3))
    e = np.array(e)
    fl_e = (nb + 32) * n * 8 / 8e12 * 1e3
    say("## The expansion pass beside it", "",
        "k_modal_expand<32>, %d columns into 32 planes of %d rows: %.3f [%.3f, %.3f] ms, byte floor (nb + 32) n 8 B at 8 TB/s %.3f ms (%.2f x)." %
        (nb, n, np.median(e), e.min(), e.max(), fl_e, np.median(e) / fl_e),
        "A group of 32 factor fields therefore costs %.3f ms of expansion + %.3f ms of stress sums." % (np.median(e), np.median(s)), "")

    # ---- a whole call
    t0 = time.time()
    lam, X, info = c.modal_basis(a.modes, batch=16, rtol=1e-6, maxit=3000)
    t_modes = time.time() - t0
    del X
    w = np.sqrt(lam)
    say("## modal_random_stress, static correction, von Mises and components", "",
        "modal_basis(%d): %.1f s wall (modes_many and the handover on the device)." % (a.modes, t_modes), "",
        "| grid points | outputs | wall s | covarianceMs (host) | factorMs (host) | passes, peak and the copies to the host, ms by device events | rank | passes | truncation | static iterations | peak von Mises (element, corner) |",
        "|---|---|---|---|---|---|---|---|---|---|---|")
    om = np.linspace(0.2 * w[0], 1.1 * w[-1], a.points)
    S = 1.0 / (1.0 + (om / w[0]) ** 2)
    for comps in (False, True):
        c.modal_random_stress(om[:50], S[:50], f, modal_damping=0.02, rtol=a.rtol, maxit=a.maxit, components=comps)          # warm-up
        t0 = time.time()
        r = c.modal_random_stress(om, S, f, modal_damping=0.02, rtol=a.rtol, maxit=a.maxit, components=comps)
        wall = time.time() - t0
        i = r["info"]
        say("| %d | %s | %.3f | %.1f | %.2f | %.2f | %d | %d | %.2e | %d | %.4e (%d, %d) |" %
            (a.points, "von Mises + components" if comps else "von Mises", wall, i["covarianceMs"], i["factorMs"], i["solveMs"], i["ranks"][0], i["passes"][0],
             i["truncation"][0], i["staticIterations"], r["peak"][0], r["peak"][1], r["peak"][2]))
    say("", "(wall includes the static solve, the load projection and the copies of the outputs to the host: %.0f MB of von Mises values, %.0f MB of components.)" %
        (ne * NQ * 8 / 1e6, ne * NQ * 6 * 8 / 1e6), "")
    c.close()


if __name__ == "__main__":
    main()
