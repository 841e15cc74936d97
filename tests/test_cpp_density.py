"""include/MeshFEMHip/MassProperties.hh and the per-element overload of Eigensolver.hh compile with plain g++ against the C ABI; on the GPU the
program computes the clamped modes of the bimaterial body and its mass properties, and they are the Python layer's on the same mesh: eigenvalues to
1e-10 relative, the mass properties and M x bit for bit -- the same kernels on the same numbers (both sides run with option deterministic 1, so
that two processes add in the same order); only the call marshalling differs."""
import os
import subprocess

import numpy as np
import pytest

import meshfem_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "facade_density"
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
    import density_util as DU
    _build()
    V, T = O.grid_tet_mesh(3, 2, 2)                      # unperturbed: the clamp is the box of the face x = min
    with open(tmp_path / "mesh.bin", "wb") as f:
        np.array([len(V), len(T)], dtype=np.int64).tofile(f)
        np.ascontiguousarray(V, dtype=np.float64).tofile(f)
        np.ascontiguousarray(T, dtype=np.int32).tofile(f)
    nev = 4
    r = subprocess.run([EXE, "0", str(tmp_path / "mesh.bin"), str(nev), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "density ok" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.bin")
    sim = Simulator(T, V, 2)
    sim.ctx.set_option("deterministic", 1)
    sim.setIsotropicMaterial(1.0, 0.3)
    sim.applyDirichletBox([-1e-9] * 3, [1e-9, 1 + 1e-9, 1 + 1e-9], [0, 0, 0], relative=True)
    rho = DU.density_field("bimaterial", T, V, 3)
    assert rho.min() == 1.0 and rho.max() == 8.0
    freq, _ = sim.vibrational_modes(nev, density=rho)
    lam = (2 * np.pi * freq) ** 2
    p = sim.massProperties()
    Mx = sim.applyMassMatrix(sim.nodes())
    assert out.size == nev + 1 + 3 + 9 + 9 + Mx.size
    err = np.abs(out[:nev] / lam - 1).max()
    print("eigenvalues: %.3e relative" % err)
    assert err <= 1e-10
    assert out[nev] == p["mass"] and np.array_equal(out[nev + 1:nev + 4], p["com"])
    assert np.array_equal(out[nev + 4:nev + 13].reshape(3, 3), p["second_moment"])
    assert np.array_equal(out[nev + 13:nev + 22].reshape(3, 3), p["inertia"])
    assert np.array_equal(out[nev + 22:].reshape(Mx.shape), Mx)
    ref = DU.mass_properties(3, sim.elements(), sim.nodes(), rho)
    assert abs(p["mass"] / ref["mass"] - 1) <= 1e-12
    sim.ctx.close()
