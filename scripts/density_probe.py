"""Record of the per-element density on one MI355X (docs/design/04_15_density.md) on the bench workload (60^3 grid -> 5.18 M quadratic tets):
  (a) the density-weighted mass assembly pass (k_assemble_gather<3, 2, MAT_MASS_RHO>) against the unit-density pass (MAT_MASS, the code of the
      commit before the feature) on the same context, launched in turns, device events per launch (mfh_time_mass_assembly);
  (b) mfh_mass_properties (two passes, each a partial-sum kernel and a one-workgroup finish, and the read-back; host clock around the call, which
      ends in a stream synchronisation) against the time to stream the node table, the connectivity and the field once per pass at the copy rate
      measured in the same process (device-to-device copy of 1 GiB: bytes read + bytes written over the time);
  (c) mfh_modes, nev 8, multigrid, clamped on x = 0, with the bimaterial field and at unit density: iterations and solve time.
Writes the measured section of profiles/r11_density.md to profiles/r11_density_measured.md (or --out); the table of kernel resources in that
file comes from the compiler, not from this script."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60, help="grid cells per axis (the bench workload: 60)")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--no-modes", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_density_measured.md"))
    a = ap.parse_args()
    import torch
    import meshfem_amd as M
    from meshfem_amd import grid
    from meshfem_amd._lib import ptr
    V, T = grid.grid_tet_mesh(a.n, a.n, a.n, [0, 0, 0], [1, 1, 1])
    c = M.Context(0)
    c.set_option("matrix_storage", 0)                  # both triangles, as mfh_modes / mfh_newmark hold them for their own duration
    c.mesh_build(T, V, 2)
    c.material_isotropic(200.0, 0.35)
    centroid_x = V[T][:, :, 0].mean(axis=1)
    rho = np.where(centroid_x < 0.5, 1.0, 8.0)
    c.set_density(rho)
    lines = ["## Measured: %d^3 grid, %d quadratic tets, %d nodes" % (a.n, c.n_elem, c.n_node), ""]

    # (a) the assembly pass
    unit, field = np.zeros(a.reps + 5), np.zeros(a.reps + 5)
    c._ck(c.lib.mfh_time_mass_assembly(c.h, a.reps + 5, ptr(unit), ptr(field)))
    unit, field = unit[5:], field[5:]
    mu, mf = float(np.median(unit)), float(np.median(field))
    lines += ["Mass assembly pass, device events per launch, the two flavours launched in turns, median of %d after 5 warm-up pairs:" % a.reps, "",
              "| pass | ms (median) | min - max |", "|---|---|---|",
              "| MAT_MASS (unit density) | %.3f | %.3f - %.3f |" % (mu, unit.min(), unit.max()),
              "| MAT_MASS_RHO (bimaterial field) | %.3f | %.3f - %.3f |" % (mf, field.min(), field.max()), "",
              "ratio density-weighted / unit: **%.3f**" % (mf / mu), ""]

    # (b) mass properties against the copy rate
    nbytes = 1 << 30
    src = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    ts = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    copy_tbs = 2 * nbytes / (float(np.median(ts)) * 1e-3) / 1e12
    del src, dst
    for _ in range(5):
        c.mass_properties()
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        p = c.mass_properties()
        ms.append((time.perf_counter() - t0) * 1e3)
    per_pass = 8 * 3 * c.n_node + 4 * c.npe * c.n_elem + 8 * c.n_elem
    floor = 2 * per_pass / (copy_tbs * 1e12) * 1e3
    lines += ["mfh_mass_properties (both passes, their finish kernels, the read-back; host clock around the call, median of %d after 5 warm-up calls):" % a.reps,
              "**%.3f ms** (min %.3f, max %.3f). Bytes per pass: node table %.1f MB + connectivity %.1f MB + field %.1f MB = %.1f MB; copy rate measured in" %
              (float(np.median(ms)), min(ms), max(ms), 24 * c.n_node / 1e6, 4 * c.npe * c.n_elem / 1e6, 8 * c.n_elem / 1e6, per_pass / 1e6),
              "this process (1 GiB device to device, read + written): %.2f TB/s; two passes at that rate: %.3f ms; ratio **%.2f**." %
              (copy_tbs, floor, float(np.median(ms)) / floor),
              "mass %.12g, centre %s" % (p["mass"], np.array2string(p["com"], precision=12)), ""]

    # (c) modes
    if not a.no_modes:
        c.set_preconditioner(M.PRECOND_MULTIGRID)
        c.bc_dirichlet_box([-1e-9] * 3, [1e-9, 1 + 1e-9, 1 + 1e-9], [0, 0, 0], relative=True)
        v, _ = c.bc_dirichlet_vars()
        c.fix_variables(v)
        rows = []
        for name, fld in (("unit density (warm-up)", None), ("unit density", None), ("bimaterial 1 : 8", rho), ("unit density", None), ("bimaterial 1 : 8", rho)):
            c.set_density(fld)
            lam, _, info = c.modes(8, rtol=1e-6, maxit=500)
            rows.append("| %s | %d | %.1f | %.1f | %.6g | %.6g |" % (name, info["iterations"], info["solve_ms"], info["setup_ms"], lam[0], lam[-1]))
        lines += ["mfh_modes, nev 8, multigrid, clamped on x = 0, rtol 1e-6, the two bodies in turns on one context:", "",
                  "| mass | iterations | solve ms | setup ms | lambda_1 | lambda_8 |", "|---|---|---|---|---|---|"] + rows + [""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))
    c.close()


if __name__ == "__main__":
    main()
