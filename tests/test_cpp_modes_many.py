"""The mfh_modes_many overload of include/MeshFEMHip/Eigensolver.hh compiles with plain g++ against the C ABI; on the GPU it returns, for 10 modes
in batches of 4 followed by 3 more in the complement of those (the continuation through `locked`), the eigenvalues and modes the Python layer
returns for the same mesh, clamp and calls: 1e-12 relative -- the same code path, only the call marshalling differs (both sides run with option
deterministic 1, so that two processes add in the same order)."""
import os
import subprocess

import numpy as np
import pytest

import meshfem_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "facade_modes_many"
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
def test_facade_matches_the_python_layer(tmp_path):
    from oracle import meshfem_oracle as O
    from meshfem_amd.linear_elasticity import Simulator
    _build()
    V, T = O.grid_tet_mesh(3, 2, 2)                      # unperturbed: the clamp is the box of the face x = min
    with open(tmp_path / "mesh.bin", "wb") as f:
        np.array([len(V), len(T)], dtype=np.int64).tofile(f)
        np.ascontiguousarray(V, dtype=np.float64).tofile(f)
        np.ascontiguousarray(T, dtype=np.int32).tofile(f)
    nev, batch, more, density = 10, 4, 3, 2.5
    r = subprocess.run([EXE, "0", str(tmp_path / "mesh.bin"), str(nev), str(batch), str(more), repr(density), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "modes ok" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.bin")
    sim = Simulator(T, V, 2)
    sim.ctx.set_option("deterministic", 1)
    sim.setIsotropicMaterial(1.0, 0.3)
    sim.applyDirichletBox([-1e-9] * 3, [1e-9, 1 + 1e-9, 1 + 1e-9], [0, 0, 0], relative=True)
    f1, m1 = sim.vibrational_modes_many(nev, density=density, batch=batch)
    assert sim.modes_many_info["batches"] == 3
    f2, m2 = sim.vibrational_modes_many(more, density=density, batch=batch, locked=m1)
    lam = (2 * np.pi * np.concatenate([f1, f2])) ** 2
    modes = np.concatenate([m1, m2])
    assert out.size == nev + more + modes.size
    assert np.abs(out[:nev + more] - lam).max() <= 1e-12 * lam.max()
    assert np.abs(out[nev + more:] - modes.reshape(-1)).max() <= 1e-9 * np.abs(modes).max()
    sim.ctx.close()
