"""The field sampler on the 40^3 grid of quadratic tets (the mesh of scripts/probe_stress_measures.py) at 10^6 query points, 90 % uniform in
the bounding box and 10 % outside it (0.01 to 1 box edge beyond a face).
    python scripts/probe_field_sampler.py [n] [out.json] [nPoints]
Run it under `rocprofv3 --kernel-trace --stats -- python scripts/probe_field_sampler.py` in a process of its own for the kernel times
(k_locate, k_closest_boundary, k_sample_field and the build kernels): Context.sample is called REPEATS times after a warm call.
On its own it reports the index build (mfh_sampler_info), the warm end-to-end median of Context.sample(P, u) (host clock around the blocking
call: points and field to the device, three kernels, values back) and the only route a user had before: the field and the mesh on the
host, a scipy cKDTree over the element centroids as the candidate filter (the K nearest centroids per point), the barycentric test of the
numpy restatement on the candidates and the P2 shape functions, on HOST_POINTS inside points, scaled to all points and labelled as scaled."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import numpy as np

import meshfem_amd as M
from meshfem_amd import grid

REPEATS = 7
HOST_POINTS = 20000
K_NEAREST = 32


def median_ms(fn):
    fn()
    ts = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return statistics.median(ts)


def host_route(V, T, en, u, P):
    """sample u at the points P on the host; returns (values, fraction of points whose element was among the candidates)"""
    import field_sampler_util as R
    from scipy.spatial import cKDTree
    tree = cKDTree(V[T].mean(axis=1))
    _, cand = tree.query(P, k=K_NEAREST)
    out = np.full((len(P), u.shape[1]), np.nan)
    found = np.zeros(len(P), dtype=bool)
    for j in range(K_NEAREST):
        todo = np.flatnonzero(~found)
        if not len(todo):
            break
        lam = R.bary_in(V, T, cand[todo, j], P[todo])
        hit = lam.min(axis=1) >= -R.CONTAIN_TOL
        idx = todo[hit]
        N = R.shape_functions(lam[hit], 2)
        out[idx] = np.einsum("pk,pkc->pc", N, u[en[cand[idx, j]]])
        found[idx] = True
    return out, found.mean()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    n_points = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
    V, T = grid.grid_tet_mesh(n, n, n, [0, 0, 0], [1, 1, 1])
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    rng = np.random.default_rng(0)
    u = rng.standard_normal((c.n_node, 3))
    n_out = n_points // 10
    P = rng.uniform(0.0, 1.0, (n_points, 3))
    axis, side = rng.integers(0, 3, n_out), rng.integers(0, 2, n_out)
    dist = 10.0 ** rng.uniform(-2, 0, n_out)
    P[np.arange(n_out), axis] = np.where(side == 1, 1.0 + dist, -dist)
    P = np.ascontiguousarray(P[rng.permutation(n_points)])
    out = {"grid": n, "elements": len(T), "nodes": c.n_node, "points": n_points, "points_outside": n_out, "components": 3, "repeats": REPEATS}
    t = time.perf_counter()
    c.sampler_build()
    out["sampler_build_call_ms"] = 1e3 * (time.perf_counter() - t)
    out["first_sample_call_ms"] = None
    t = time.perf_counter()
    vals = c.sample(P, u)
    out["first_sample_call_ms"] = 1e3 * (time.perf_counter() - t)
    out["sampler_info"] = c.sampler_info()
    out["sample_call_ms"] = median_ms(lambda: c.sample(P, u))
    out["locate_call_ms"] = median_ms(lambda: c.locate(P))
    inside = np.flatnonzero(c.contains(P))
    out["points_contained"] = int(len(inside))
    try:
        import scipy  # noqa: F401
        sub = inside[:HOST_POINTS]
        en = c.elem_nodes()
        Vh, Th = np.ascontiguousarray(V), np.ascontiguousarray(T)
        t = time.perf_counter()
        hv, frac = host_route(Vh, Th, en, u, P[sub])
        ms = 1e3 * (time.perf_counter() - t)
        ok = ~np.isnan(hv[:, 0])
        out["host_route"] = {"points": int(len(sub)), "ms": ms, "candidates_per_point": K_NEAREST, "fraction_found": float(frac),
                             "max_abs_difference_to_device": float(np.abs(hv[ok] - vals[sub][ok]).max()),
                             "scaled_to_all_points_ms": ms * n_points / len(sub),
                             "note": "inside points only (no closest-point search on the host), cKDTree build included, scaled linearly"}
        out["host_over_device_scaled"] = out["host_route"]["scaled_to_all_points_ms"] / out["sample_call_ms"]
    except ImportError:
        out["host_route"] = "scipy does not import here: not measured"
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
