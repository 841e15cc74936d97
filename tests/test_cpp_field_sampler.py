"""include/MeshFEMHip/FieldSampler.hh compiles with plain g++ against the C ABI; on the GPU its five methods over a quadratic Simulator and
over a raw mesh return what the numpy restatement (tests/field_sampler_util.py) gives: the bounds of tests/test_gpu_field_sampler.py."""
import os
import subprocess

import numpy as np
import pytest

import meshfem_amd as M
import field_sampler_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "facade_field_sampler"
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
@pytest.mark.timeout(120)
def test_facade_matches_the_restatement(tmp_path):
    from oracle import meshfem_oracle as O
    _build()
    V, T = O.grid_tet_mesh(3, 2, 2)
    V = np.ascontiguousarray(V + 0.08 * np.random.default_rng(3).standard_normal(V.shape))
    T = np.ascontiguousarray(T)
    with open(tmp_path / "mesh.bin", "wb") as f:
        np.array([len(V), len(T)], dtype=np.int64).tofile(f)
        V.tofile(f)
        np.ascontiguousarray(T, dtype=np.int32).tofile(f)
    c = M.Context(0)                                    # the library's own numbering of the quadratic nodes
    c.mesh_build(T, V, 2)
    en, npos = c.elem_nodes(), c.node_positions()
    c.close()
    rng = np.random.default_rng(4)
    e = rng.integers(0, len(T), 60)
    Pin = np.einsum("pk,pka->pa", rng.dirichlet(np.ones(4), 60), V[T[e]])
    Pin = Pin[R.bary_in(V, T, e, Pin).min(axis=1) > 1e-6]
    mn, mx = V.min(0), V.max(0)
    Pout = mx + (mx - mn) * rng.uniform(0.05, 1.0, (20, 3)) * np.where(rng.integers(0, 2, (20, 3)) == 1, 1.0, -0.2)
    Pout = Pout[R.locate(V, T, Pout)[0] < 0]
    P = np.concatenate([Pin, Pout])
    n, na = len(P), len(Pin)
    P.tofile(tmp_path / "P.bin")
    field = np.stack([1.0 + npos @ np.array([1.0, -2.0, 0.5]) + npos[:, 0] * npos[:, 1], npos[:, 2] ** 2 - npos[:, 0]], axis=1)
    field.tofile(tmp_path / "f.bin")
    r = subprocess.run([EXE, "0", str(tmp_path / "mesh.bin"), str(tmp_path / "P.bin"), str(tmp_path / "f.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "field sampler ok" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.bin")
    sizes = [n, 4 * n, 3 * n, n, n, n, n, 2 * n, n, n]
    assert out.size == sum(sizes)
    I, B, Cl, d2, NI, nd2, inside, s, rawI, rawS = np.split(out, np.cumsum(sizes)[:-1])
    I, NI, rawI = I.astype(int), NI.astype(int), rawI.astype(int)
    B, Cl, s = B.reshape(n, 4), Cl.reshape(n, 3), s.reshape(n, 2)
    rI, rB, rC, rd2 = R.locate_full(V, T, P)
    diag2 = np.linalg.norm(mx - mn) ** 2
    assert np.array_equal(I[:na], rI[:na]) and np.abs(B[:na] - rB[:na]).max() <= 1e-10
    assert np.abs(Cl - rC).max() <= 1e-12 * diag2 and np.abs(d2 - rd2).max() <= 1e-12 * diag2
    assert np.all(np.sqrt(R.dist2_to_elements(V, T, I[na:], P[na:])) - np.sqrt(rd2[na:]) <= 1e-12 * np.sqrt(diag2))
    assert np.array_equal(inside.astype(bool), rd2 <= 1e-20) and inside[:na].all() and not inside[na:].any()
    q = lambda X: np.stack([1.0 + X @ np.array([1.0, -2.0, 0.5]) + X[:, 0] * X[:, 1], X[:, 2] ** 2 - X[:, 0]], axis=1)
    assert np.abs(s - q(Cl)).max() <= 1e-12 * np.abs(field).max()
    rnode, rnd2, lead = R.closest_node(en, npos, 2, rI, rB, P)
    ok = lead > 1e-9
    ok[na:] &= I[na:] == rI[na:]
    assert ok[:na].mean() >= 0.9 and np.array_equal(NI[ok], rnode[ok]) and np.abs(nd2[ok] - rnd2[ok]).max() <= 1e-12 * diag2
    assert np.array_equal(rawI[:na], rI[:na])
    lin = lambda X: X[:, 0] + 2.0 * X[:, 1] - X[:, 2]
    assert np.abs(rawS - lin(Cl)).max() <= 1e-12 * np.abs(lin(V)).max()
