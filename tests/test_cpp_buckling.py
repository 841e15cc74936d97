"""include/MeshFEMHip/Buckling.hh compiles with plain g++ against the C ABI; on the GPU the program computes the load factors of the unperturbed
3 x 2 x 10 linear column under unit axial compression and Kg x, and they are the Python layer's on the same mesh: factors to 1e-10 relative, Kg x
bit for bit -- the same kernels on the same numbers (both sides run with option deterministic 1); only the call marshalling differs."""
import os
import subprocess

import numpy as np
import pytest

import meshfem_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "facade_buckling"
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
    V, T = O.grid_tet_mesh(3, 2, 10)                     # unperturbed: the clamp is the box of the face z = min
    with open(tmp_path / "mesh.bin", "wb") as f:
        np.array([len(V), len(T)], dtype=np.int64).tofile(f)
        np.ascontiguousarray(V, dtype=np.float64).tofile(f)
        np.ascontiguousarray(T, dtype=np.int32).tofile(f)
    nev = 3
    r = subprocess.run([EXE, "0", str(tmp_path / "mesh.bin"), str(nev), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "buckling ok" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.bin")
    sim = Simulator(T, V, 1)
    sim.ctx.set_option("deterministic", 1)
    sim.setIsotropicMaterial(1.0, 0.3)
    sim.applyDirichletBox([-1e-9] * 3, [1 + 1e-9, 1 + 1e-9, 1e-9], [0, 0, 0], relative=True)
    sigma = np.zeros((len(T), 6))
    sigma[:, 2] = -1.0
    sim.setPrestress(sigma)
    v, _ = sim.ctx.bc_dirichlet_vars()
    sim.ctx.fix_variables(v)
    fac, X, info = sim.ctx.buckling(nev, rtol=1e-6, maxit=3000)
    Gx = sim.applyGeometricStiffness(sim.nodes())
    assert out.size == nev + Gx.size
    err = np.abs(out[:nev] / fac - 1).max()
    print("factors %s: %.3e relative" % (fac, err))
    assert info["nBuckling"] == nev and err <= 1e-10
    assert np.array_equal(out[nev:].reshape(Gx.shape), Gx)
    sim.ctx.close()
