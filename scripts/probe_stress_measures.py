"""The stress-measure entry points on the 40^3 grid of quadratic tets (the mesh of scripts/probe_spmv_kron.py).
    python scripts/probe_stress_measures.py [n] [out.json]
Run it under `rocprofv3 --kernel-trace --stats -- python scripts/probe_stress_measures.py` for the kernel times: every entry point is
called REPEATS times after a warm call, so the stats hold one average per kernel (k_stress_measures appears with two call counts' worth of
launches: von Mises only and eigenvalues only are told apart by running the script with MEASURE=vm or MEASURE=eig).
On its own it reports end-to-end medians (host clock around the blocking calls, warm, same process):
  peak_device_ms   peak_von_mises(u): u to the device, two-stage reduction, two numbers back
  peak_host_ms     what a caller did before: strain_field(u, stress=True) to the host, von Mises and argmax in numpy"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import meshfem_amd as M
from meshfem_amd import grid

REPEATS = 7


def median_ms(fn):
    fn()
    ts = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return statistics.median(ts)


def host_peak(c, u):
    s = c.strain_field(u, True)
    d = s[..., :3] - s[..., :3].mean(axis=-1, keepdims=True)
    vm = np.sqrt(1.5 * ((d * d).sum(axis=-1) + 2.0 * (s[..., 3:] ** 2).sum(axis=-1)))
    i = int(np.argmax(vm))
    return float(vm.reshape(-1)[i]), i


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    which = os.environ.get("MEASURE", "all")
    V, T = grid.grid_tet_mesh(n, n, n, [0, 0, 0], [1, 1, 1])
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    c.material_isotropic(200.0, 0.35)
    u = np.random.default_rng(0).standard_normal((c.n_node, 3))
    out = {"grid": n, "elements": len(T), "nodes": c.n_node, "vertices": c.n_vert, "corners": 4 * len(T), "repeats": REPEATS}
    if which in ("all", "vm"):
        out["von_mises_call_ms"] = median_ms(lambda: c.von_mises(u))
    if which in ("all", "eig"):
        out["principal_values_call_ms"] = median_ms(lambda: c.principal_values(u))
    if which == "all":
        sig = c.strain_field(u, True)
        out["strain_field_call_ms"] = median_ms(lambda: c.strain_field(u, True))
        out["vertex_average_c6_call_ms"] = median_ms(lambda: c.vertex_averaged_field(sig))
        out["vertex_averaged_stress_call_ms"] = median_ms(lambda: c.vertex_averaged_stress(u))
        out["peak_device_ms"] = median_ms(lambda: c.peak_von_mises(u))
        out["peak_host_ms"] = median_ms(lambda: host_peak(c, u))
        pd, ph = c.peak_von_mises(u), host_peak(c, u)
        out["peak_device"], out["peak_host"] = list(pd), list(ph)
        out["peak_ratio_host_over_device"] = out["peak_host_ms"] / out["peak_device_ms"]
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
