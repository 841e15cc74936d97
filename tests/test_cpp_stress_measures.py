"""include/MeshFEMHip/VonMises.hh and FieldPostProcessing.hh compile with plain g++ against the C ABI; on the GPU their free functions over a
quadratic Simulator (vonMises, eigenvalues, eigenDecomposition, vonMisesStress, principalStresses, peakVonMises, vertexAveragedField,
vertexAveragedStress) return what the numpy restatement of the reference's routines (tests/stress_measures_util.py) gives for the stress
field the same Simulator reports: 1e-12 max|sigma|, the bound of tests/test_gpu_stress_measures.py."""
import os
import subprocess

import numpy as np
import pytest

import meshfem_amd as M
import stress_measures_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "facade_stress_measures"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)


def _build():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cc")
    libdir = os.path.dirname(M.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", EXE,
                           "-L", libdir, "-lmeshfem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])


def test_headers_compile_and_throw_without_device():
    _build()
    r = subprocess.run([EXE, "-1"], capture_output=True, text=True)
    assert r.returncode == 3 and "runtime_error" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_facade_matches_the_restatement(tmp_path):
    from oracle import meshfem_oracle as O
    _build()
    V, T = O.grid_tet_mesh(3, 2, 2)
    V = V + 0.08 * np.random.default_rng(3).standard_normal(V.shape)
    with open(tmp_path / "mesh.bin", "wb") as f:
        np.array([len(V), len(T)], dtype=np.int64).tofile(f)
        np.ascontiguousarray(V, dtype=np.float64).tofile(f)
        np.ascontiguousarray(T, dtype=np.int32).tofile(f)
    c = M.Context(0)                                    # the library's own numbering of the quadratic nodes
    c.mesh_build(T, V, 2)
    n_node, n_elem, n_vert = c.n_node, c.n_elem, c.n_vert
    cn, vol = c.elem_nodes()[:, :4], c.elem_volumes()
    c.close()
    u = np.random.default_rng(4).standard_normal((n_node, 3))
    u.tofile(tmp_path / "u.bin")
    r = subprocess.run([EXE, "0", str(tmp_path / "mesh.bin"), str(tmp_path / "u.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "stress measures ok" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.bin")
    nc = 4 * n_elem
    sizes = [6 * nc, nc, 3 * nc, nc, 3 * nc, 2, 6 * n_vert, 6 * n_vert, n_vert]
    assert out.size == sum(sizes)
    sig, vm, ev, vm_f, ev_f, peak, avg, avg_one, avg_s = np.split(out, np.cumsum(sizes)[:-1])
    sig = sig.reshape(n_elem, 4, 6)
    tol = 1e-12 * np.abs(sig).max()
    assert np.abs(sig).max() > 0
    ref_vm, ref_ev = R.von_mises(sig).reshape(-1), R.eigenvalues(sig).reshape(-1)
    assert np.abs(vm - ref_vm).max() <= tol and np.abs(vm_f - ref_vm).max() <= tol
    assert np.abs(ev - ref_ev).max() <= tol and np.abs(ev_f - ref_ev).max() <= tol
    assert peak[0] == vm_f.max() and int(peak[1]) == int(np.argmax(vm_f))
    ref_avg = R.vertex_averaged(cn, vol, sig, n_vert).reshape(-1)
    assert np.abs(avg - ref_avg).max() <= tol and np.array_equal(avg_one, avg)
    per_elem = 1.0 + 0.25 * (np.arange(n_elem) % 5)
    assert np.abs(avg_s - R.vertex_averaged(cn, vol, per_elem[:, None], n_vert)).max() <= 1e-12 * per_elem.max()
