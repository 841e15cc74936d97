"""Record of the volume-load kernels on one MI355X (k_body_force_load, k_stress_field_load; docs/design/04_14_volume_loads.md): on the bench workload
(60^3 grid -> 5.18 M quadratic tets) every flavour is called with device pointers and timed with device events on the context's stream (median of --reps
calls after warm-up), then set beside two yardsticks:
  (a) the atomic k_constant_strain_load on the same mesh -- the scatter kernel the STRAIN flavour replaces when it is fed one strain everywhere. It has no
      device-pointer entry, so its time (and, as a cross-check, the new kernels' own) comes from a rocprofv3 kernel trace of a child process (--worker);
  (b) the bytes the kernel must move (DoF-pair list, element records, fields, out) at the streaming rate profiles/r06_summary.md records for the box
      (triad, 5.82 TB/s).
Writes profiles/r10_volume_loads.md (or --out)."""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STREAM_TBS = 5.82          # profiles/r06_summary.md: triad measured on the box
GEO_ISO_STRIDE = 16        # doubles per element record of an isotropic material (mfh_internal.hh)


def _context(n):
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(n, n, n, [0, 0, 0], [1, 1, 1])
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    c.material_isotropic(200.0, 0.35)
    return c


def _fields(c, seed=1):
    rng = np.random.default_rng(seed)
    return dict(b=rng.standard_normal(3), b_elem=rng.standard_normal((c.n_elem, 3)), b_node=rng.standard_normal((c.n_node, 3)),
                rho=rng.uniform(0.5, 2.0, c.n_elem), sigma=rng.standard_normal((c.n_elem, 6)), eps=np.tile(rng.standard_normal(6), (c.n_elem, 1)))


def _flavours():
    from meshfem_amd import _lib as L
    # (name, entry, kind, field, density, stressOut, kernel name in a trace)
    return [("body force CONSTANT", "body", L.BODY_CONSTANT, "b", False, False, "k_body_force_load<3, 2, 0>"),
            ("body force CONSTANT, density", "body", L.BODY_CONSTANT, "b", True, False, "k_body_force_load<3, 2, 0>"),
            ("body force ELEMENT, density", "body", L.BODY_ELEMENT, "b_elem", True, False, "k_body_force_load<3, 2, 1>"),
            ("body force NODE, density", "body", L.BODY_NODE, "b_node", True, False, "k_body_force_load<3, 2, 2>"),
            ("stress field STRESS", "stress", L.FIELD_LOAD_STRESS, "sigma", False, False, "k_stress_field_load<3, 2, 0, false>"),
            ("stress field STRAIN (one strain everywhere)", "stress", L.FIELD_LOAD_STRAIN, "eps", False, False, "k_stress_field_load<3, 2, 0, true>"),
            ("stress field STRAIN + stressOut", "stress", L.FIELD_LOAD_STRAIN, "eps", False, True, "k_stress_field_load<3, 2, 0, true>")]


def _must_move(c, fl):
    """bytes: the pair list (one pointer per DoF, one code per (element, node) pair), the part of the element records the kernel reads (the whole
    record for the stress-field load; for a body force the 64-byte line that holds the volume), the fields, out"""
    from meshfem_amd import _lib as L
    _, entry, kind, field, dens, sout, _ = fl
    pairs = 4 * (c.n_dof + 1) + 4 * c.n_elem * 10
    out = 8 * 3 * c.n_dof
    if entry == "body":
        f = {L.BODY_CONSTANT: 0, L.BODY_ELEMENT: 24 * c.n_elem, L.BODY_NODE: 24 * c.n_node + 40 * c.n_elem}[kind]      # NODE: b and the node table
        return pairs + 64 * c.n_elem + f + (8 * c.n_elem if dens else 0) + out
    return pairs + 8 * GEO_ISO_STRIDE * c.n_elem + 48 * c.n_elem * (2 if sout else 1) + out


def worker(n, reps):
    """the calls a kernel trace is taken of: the atomic constant-strain load through its host entry, every new flavour through the device entry"""
    import torch
    from meshfem_amd import _lib as L
    from meshfem_amd._lib import ptr
    c = _context(n)
    f = _fields(c)
    for _ in range(reps):
        c.constant_strain_load(f["eps"][0])                   # fresh context, no operator lists: k_constant_strain_load
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in f.items() if k != "b"}
    out = torch.empty(c.n_dof * 3, dtype=torch.float64, device="cuda")
    sig = torch.empty(c.n_elem * 6, dtype=torch.float64, device="cuda")
    b = np.ascontiguousarray(f["b"])
    for fl in _flavours():
        for _ in range(reps):
            _call(c, fl, dev, b, out, sig, L, ptr)
    torch.cuda.synchronize()
    c.close()


def _call(c, fl, dev, b, out, sig, L, ptr):
    _, entry, kind, field, dens, sout, _ = fl
    if entry == "body":
        bp = ptr(b) if kind == L.BODY_CONSTANT else dev[field].data_ptr()
        c._ck(c.lib.mfh_body_force_load(c.h, kind, bp, dev["rho"].data_ptr() if dens else None, L.LOAD_ON_DEVICE, out.data_ptr()))
    else:
        c._ck(c.lib.mfh_stress_field_load(c.h, kind, dev[field].data_ptr(), sig.data_ptr() if sout else None, L.LOAD_ON_DEVICE, out.data_ptr()))


def trace(n, reps):
    """{kernel name (template arguments kept): median ms} from a rocprofv3 kernel trace of the worker"""
    d = tempfile.mkdtemp(prefix="volume_loads_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--worker",
           "--n", str(n), "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return None, (r.stdout + r.stderr)[-2000:]
    times = {}
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            name = re.sub(r"\(.*", "", row.get("Kernel_Name", "").replace("(anonymous namespace)::", "").replace("mfh::k::", "").replace("void ", ""))
            times.setdefault(name, []).append((float(row["End_Timestamp"]) - float(row["Start_Timestamp"])) * 1e-6)
    return {k: (float(np.median(v[len(v) // 4:])), len(v)) for k, v in times.items()}, ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60, help="grid cells per axis (the bench workload: 60)")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_volume_loads.md"))
    a = ap.parse_args()
    if a.worker:
        worker(a.n, max(4, a.reps // 3))
        return
    traced, why = (None, "skipped") if a.no_trace else trace(a.n, a.reps)      # before this process opens the device
    import torch
    from meshfem_amd import _lib as L
    from meshfem_amd._lib import ptr
    c = _context(a.n)
    f = _fields(c)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in f.items() if k != "b"}
    out = torch.empty(c.n_dof * 3, dtype=torch.float64, device="cuda")
    sig = torch.empty(c.n_elem * 6, dtype=torch.float64, device="cuda")
    b = np.ascontiguousarray(f["b"])
    stream = torch.cuda.ExternalStream(c.stream())
    lines = ["# Volume loads on one MI355X: %d^3 grid, %d quadratic tets, %d nodes" % (a.n, c.n_elem, c.n_node), "",
             "Lane mapping: one lane per DoF row walks the row's (element, local node) pairs in list order and stores its dim values once; 256 lanes per",
             "workgroup, at most 2048 workgroups, grid-stride beyond. No atomics. Device-pointer calls, device events on the context's stream around each",
             "call (kernel + launch), median of %d after 5 warm-up calls; must-move bytes at %.2f TB/s (the triad of profiles/r06_summary.md)." % (a.reps, STREAM_TBS), ""]
    rows, strain_ms = [], None
    for fl in _flavours():
        for _ in range(5):
            _call(c, fl, dev, b, out, sig, L, ptr)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _call(c, fl, dev, b, out, sig, L, ptr)
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med, lo, hi = float(np.median(ms)), float(np.min(ms)), float(np.max(ms))
        gb = _must_move(c, fl) / 1e9
        floor = gb / (STREAM_TBS * 1e3) * 1e3
        tr = traced.get(fl[6]) if traced else None
        if fl[0].startswith("stress field STRAIN (one"):
            strain_ms = med
        rows.append("| %s | %.3f | %.3f - %.3f | %s | %.3f | %.3f | %.2f |" % (fl[0], med, lo, hi, "%.3f" % tr[0] if tr else "n/a", gb, floor, med / floor))
    lines += ["| flavour | ms (events, median) | min - max | ms (kernel trace, median) | must-move GB | ms at the streaming rate | ratio |", "|---|---|---|---|---|---|---|"] + rows + [""]
    old = None
    if traced:
        old = next((v for k, v in traced.items() if k.startswith("k_constant_strain_load")), None)
    lines += ["## Yardstick (a): the atomic k_constant_strain_load", ""]
    if old and strain_ms:
        lines += ["k_constant_strain_load on the same mesh (fresh context, kernel trace, median of %d launches): **%.3f ms**. The gather STRAIN flavour fed one" % (old[1], old[0]),
                  "strain everywhere: **%.3f ms** (events) -- %s." % (strain_ms, "no slower: accepted" if strain_ms <= old[0] else "SLOWER than the atomic kernel, see below"), ""]
    else:
        lines += ["not measured: the kernel trace failed (%s)" % why.strip().replace("\n", " ")[-400:], ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))
    c.close()


if __name__ == "__main__":
    main()
