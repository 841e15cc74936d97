"""prestressedModes / applyTangentStiffness of include/MeshFEMHip/Buckling.hh compile with plain g++ against the C ABI; on the GPU the program
computes the eigenvalues of the unperturbed 3 x 2 x 10 linear column under 0.5 and 0.55 of its critical axial compression (the second call started
from the shapes of the first) and (K + s Kg) x, and they are the Python layer's on the same mesh: eigenvalues to 1e-10 relative, the product bit
for bit -- the same kernels on the same numbers (both sides run with option deterministic 1); only the call marshalling differs."""
import os
import subprocess

import numpy as np
import pytest

import meshfem_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "facade_prestressed_modes"
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
    sim = Simulator(T, V, 1)
    sim.ctx.set_option("deterministic", 1)
    sim.setIsotropicMaterial(1.0, 0.3)
    sim.applyDirichletBox([-1e-9] * 3, [1 + 1e-9, 1 + 1e-9, 1e-9], [0, 0, 0], relative=True)
    sigma = np.zeros((len(T), 6))
    sigma[:, 2] = -1.0
    sim.setPrestress(sigma)
    v, _ = sim.ctx.bc_dirichlet_vars()
    sim.ctx.fix_variables(v)
    cr = sim.ctx.buckling(1, rtol=1e-6, maxit=3000)[0][0]
    s1, s2 = float(0.5 * cr), float(0.55 * cr)           # (plain floats: their repr is what the program parses)
    r = subprocess.run([EXE, "0", str(tmp_path / "mesh.bin"), str(nev), repr(s1), repr(s2), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "prestressed modes ok" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.bin")
    lam1, X1, _ = sim.ctx.modes_prestressed(nev, s1, rtol=1e-6, maxit=3000)
    lam2, _, _ = sim.ctx.modes_prestressed(nev, s2, x0=X1, rtol=1e-6, maxit=3000)
    Tx = sim.ctx.tangent_apply(sim.nodes(), s1)
    assert out.size == 2 * nev + Tx.size
    err = max(np.abs(out[:nev] / lam1 - 1).max(), np.abs(out[nev:2 * nev] / lam2 - 1).max())
    print("critical factor %.6g; lambda %s -> %s: %.3e relative; %s" % (cr, lam1, lam2, err, r.stdout.strip().splitlines()[0]))
    assert np.all(lam1 > 0) and np.all(lam2[0] < lam1[0]) and err <= 1e-10
    assert np.array_equal(out[2 * nev:].reshape(Tx.shape), Tx)
    sim.ctx.close()
