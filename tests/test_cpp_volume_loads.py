"""include/MeshFEMHip/VolumeLoads.hh and Simulator::perElementStressFieldLoad compile with plain g++ against the C ABI; on the GPU the program repeats the
hanging-column and free-expansion checks of tests/test_gpu_volume_loads.py (same bars: 1e-9 of the scale, the closed forms lie in the P2 space) and
writes a body-force load and a stress-field load that equal the Python layer's bit for bit -- the same kernels on the same numbers, gathered in a fixed
order without atomics; only the call marshalling differs."""
import os
import subprocess

import numpy as np
import pytest

import meshfem_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "facade_volume_loads"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)


def _build():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cc")
    libdir = os.path.dirname(M.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", EXE,
                           "-L", libdir, "-lmeshfem_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])


def test_header_compiles_and_throws_without_device():
    _build()
    r = subprocess.run([EXE, "-1"], capture_output=True, text=True)
    assert r.returncode == 3 and "runtime_error" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_facade_checks_and_matches_the_python_layer(tmp_path):
    from meshfem_amd import grid
    from meshfem_amd.linear_elasticity import Simulator
    _build()
    L_ = 3.0
    V, T = grid.grid_tet_mesh(2, 2, 4, [0, 0, 0], [1, 1, L_])
    with open(tmp_path / "mesh.bin", "wb") as f:
        np.array([len(V), len(T)], dtype=np.int64).tofile(f)
        np.ascontiguousarray(V, dtype=np.float64).tofile(f)
        np.ascontiguousarray(T, dtype=np.int32).tofile(f)
    r = subprocess.run([EXE, "0", str(tmp_path / "mesh.bin"), repr(L_), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and all(s in r.stdout for s in ("column ok", "expansion ok", "volume loads ok")), r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.bin")
    sim = Simulator(T, V, 2)
    sim.setIsotropicMaterial(50.0, 0.3)
    x = sim.nodes()
    b = np.stack([x[:, 0] * x[:, 1], x[:, 2], x[:, 0] + 2.0 * x[:, 1]], axis=1)
    e = np.arange(sim.numElements())
    density = 1.0 + 0.25 * (e % 3)
    sigma = ((7 * e[:, None] + 3 * np.arange(6)[None, :]) % 11) / 11.0 - 0.5
    want = np.concatenate([sim.bodyForceLoad(b, density).reshape(-1), sim.perElementStressFieldLoad(sigma).reshape(-1)])
    assert out.size == want.size and np.abs(want).max() > 0
    assert np.array_equal(out, want)
    sim.ctx.close()
