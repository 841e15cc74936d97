"""k_spmv_kron<3> against k_spmv<3> on one block pattern: 40^3 grid of quadratic tets.
    python scripts/probe_spmv_kron.py [n] [out.json]
Same process, warm, median of REPEATS timings of REPS back-to-back launches each (HIP events, mfh_time_spmv_kernel).
  kron   : MFH_OP_MASS_VECTOR, one double per block (k_spmv_kron<3>)
  dense  : the same block pattern with dense 3 x 3 blocks through k_spmv<3> -- the assembled elasticity K of the same context with both
           triangles stored (what k_spmv<3> costs does not depend on the values: m I stored densely moves the same bytes). A matrix loaded
           with mfh_matrix_set_upper_triplets has 1 x 1 blocks and runs k_spmv<1>, so it cannot stand in for the dense-block kernel.
  scalar : MFH_OP_MASS through k_spmv<1>, times 3 (one product per component: what callers did before)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import meshfem_amd as M
from meshfem_amd import grid

REPS, REPEATS = 20, 9


def timed(c):
    c.time_spmv_kernel(REPS)                       # warm: lists, first launches
    return statistics.median(c.time_spmv_kernel(REPS) for _ in range(REPEATS))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    V, T = grid.grid_tet_mesh(n, n, n, [0, 0, 0], [1, 1, 1])
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    c.set_option("matrix_free", 0)
    c.set_option("matrix_storage", 0)
    out = {"grid": n, "elements": len(T), "nodes": c.n_node, "reps": REPS, "repeats": REPEATS}
    c.set_operator(M.OP_MASS_VECTOR)
    c.assemble()
    out["blocks"] = c.matrix_info()[2]
    out["kron_ms"] = timed(c)
    c.set_operator(M.OP_ELASTICITY)
    c.material_isotropic(200.0, 0.35)
    c.assemble()
    assert c.matrix_info()[2] == out["blocks"] and not c.matrix_storage()[0]
    out["dense_ms"] = timed(c)
    c.set_operator(M.OP_MASS)
    c.assemble()
    out["scalar_x3_ms"] = 3 * timed(c)
    out["kron_over_dense"] = out["kron_ms"] / out["dense_ms"]
    # Compulsory traffic only: values + column indices once, x once, y once. rowPtr / chunkRow and every repeated gather of an x row that
    # misses the caches come on top, so the bytes and the GB/s below are LOWER bounds on what the kernels moved.
    nb, nn = out["blocks"], c.n_node
    out["min_bytes_kron"] = nb * (8 + 4) + 2 * nn * 24
    out["min_bytes_dense"] = nb * (72 + 4) + 2 * nn * 24
    out["min_GBps_kron"] = out["min_bytes_kron"] / out["kron_ms"] / 1e6
    out["min_GBps_dense"] = out["min_bytes_dense"] / out["dense_ms"] / 1e6
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)
    assert out["kron_ms"] <= out["dense_ms"], "k_spmv_kron<3> is slower than k_spmv<3> on the same pattern"


if __name__ == "__main__":
    main()
