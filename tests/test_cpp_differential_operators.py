"""include/MeshFEMHip/DifferentialOperators.hh compiles with plain g++ against the C ABI; on the GPU its forced-degree-1 operators on a
quadratic Simulator (construct_vector_valued<1>, MassMatrix::construct<1>, Laplacian::construct<1>, the lumped diagonal) are the oracle's
on the linear mesh of the same vertices, entry for entry (1e-13 max|ref|; 1e-14 lumped)."""
import os
import subprocess

import numpy as np
import pytest

import meshfem_amd as M
from oracle import meshfem_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "facade_differential_operators"
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


def _expand(s, N):
    i = (N * s.i[:, None] + np.arange(N)[None, :]).reshape(-1)
    j = (N * s.j[:, None] + np.arange(N)[None, :]).reshape(-1)
    v = np.repeat(s.v, N)
    order = np.lexsort((i, j))
    return O.TripletMatrix.from_arrays(N * s.m, N * s.n, i[order], j[order], v[order])


@pytest.mark.gpu
def test_forced_p1_operators_match_oracle(tmp_path):
    _build()
    V, T = O.grid_tet_mesh(3, 2, 2)
    V = V + 0.08 * np.random.default_rng(3).standard_normal(V.shape)
    with open(tmp_path / "mesh.bin", "wb") as f:
        np.array([len(V), len(T)], dtype=np.int64).tofile(f)
        np.ascontiguousarray(V, dtype=np.float64).tofile(f)
        np.ascontiguousarray(T, dtype=np.int32).tofile(f)
    m1 = O.FEMMesh(T, V, 1)
    ms = O.mass_triplets(m1).sum_repeated()
    ms.dump_binary(str(tmp_path / "mass_p1.bin"))
    _expand(ms, 3).dump_binary(str(tmp_path / "mass_vector_p1.bin"))
    O.laplacian_triplets(m1).sum_repeated().dump_binary(str(tmp_path / "laplacian_p1.bin"))
    _expand(O.mass_triplets(m1, lumped=True), 3).dump_binary(str(tmp_path / "mass_vector_p1_lumped.bin"))
    r = subprocess.run([EXE, "0", str(tmp_path / "mesh.bin"), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "differential operators ok" in r.stdout, r.stdout + r.stderr
