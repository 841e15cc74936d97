"""modalRandomStress and responseSpectrumStress of include/MeshFEMHip/Harmonic.hh compile with plain g++ against the C ABI; on the GPU, over a
quadratic Simulator clamped on one face and pulled on the opposite one, they return what the Python layer's randomStress and responseSpectrumStress
return for the same mesh, conditions, mode count, grid and spectrum: 1e-12 relative -- the same code path, only the call marshalling differs (both
sides run with option deterministic 1, so that two processes add in the same order)."""
import os
import subprocess

import numpy as np
import pytest

import meshfem_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "facade_modal_stress"
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
    from meshfem_amd import _lib as L
    from meshfem_amd.linear_elasticity import Simulator
    _build()
    V, T = O.grid_tet_mesh(3, 2, 2)                      # unperturbed: the clamp and the loaded face are boxes of the faces x = min / max
    with open(tmp_path / "mesh.bin", "wb") as f:
        np.array([len(V), len(T)], dtype=np.int64).tofile(f)
        np.ascontiguousarray(V, dtype=np.float64).tofile(f)
        np.ascontiguousarray(T, dtype=np.int32).tofile(f)
    density = 2.5
    r = subprocess.run([EXE, "0", str(tmp_path / "mesh.bin"), repr(density), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "modal stress ok" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.bin")
    omegas = 0.02 + 0.015 * np.arange(40.0)
    S = 1.0 / (1.0 + omegas * omegas)
    sim = Simulator(T, V, 2)
    sim.ctx.set_option("deterministic", 1)
    sim.setIsotropicMaterial(1.0, 0.3)
    sim.applyDirichletBox([-1e-9] * 3, [1e-9, 1 + 1e-9, 1 + 1e-9], [0, 0, 0], relative=True)
    sim.applyNeumannBox([1 - 1e-9, -1e-9, -1e-9], [1 + 1e-9] * 3, [0, 0, -1.0], kind=L.NEUMANN_TRACTION, relative=True)
    res = sim.randomStress(omegas, S, n_modes=8, density=density, modal_damping=0.03, components=True, rtol=1e-10, maxit=10000)
    assert sim.random_stress_info["staticSolves"] == 1 and sim.random_stress_info["nb"] == 9 and sim.modal_basis_info["nModes"] == 8
    assert res["von_mises"].shape == (len(T), 4) and res["components"].shape == (len(T), 4, 6) and res["von_mises"].min() >= 0.0 and res["von_mises"].max() > 0.0
    lam = (2.0 * np.pi * sim.modal_frequencies) ** 2
    rs = sim.responseSpectrumStress(2, lambda w, z: 0.3 / (w * w) * (1.0 + z), modal_damping=0.05, rule="cqc", n_modes=8, density=density)
    parts = [res["von_mises"].reshape(-1), res["components"].reshape(-1), np.array(res["peak"], dtype=np.float64), res["cov"].reshape(-1), lam,
             rs["von_mises"].reshape(-1), np.array(rs["peak"], dtype=np.float64), sim.spectrum_stress_info["gamma"]]
    names = ("von Mises", "components", "peak", "cov", "lambda", "spectrum von Mises", "spectrum peak", "gamma")
    assert out.size == sum(p.size for p in parts)
    at = 0
    for name, w in zip(names, parts):
        g = out[at:at + w.size]
        at += w.size
        assert np.abs(g - w).max() <= 1e-12 * np.abs(w).max(), name
    sim.ctx.close()
