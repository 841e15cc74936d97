"""Checks of the compiled `field_sampler` module (meshfem_amd/pybind), run as a script in its own interpreter by
tests/test_pybind_field_sampler.py.
    python tests/pybind_field_sampler_checks.py cpu | gpu"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import meshfem_amd.pybind as pb                      # noqa: E402
from meshfem_amd.pybind import build as pbuild       # noqa: E402

pbuild.build(verbose=False)
sys.path.insert(0, pb.PATH)
import mesh as cmesh                                 # noqa: E402
import field_sampler as cfs                          # noqa: E402
import field_sampler_util as R                       # noqa: E402
from oracle import meshfem_oracle as O               # noqa: E402

assert cfs.__file__.endswith(".so") and os.path.dirname(cfs.__file__) == pb.PATH, cfs.__file__

# argument names and defaults of the reference's class (src/python_bindings/field_sampler.cc)
SIGNATURES = {
    "closestElementAndPoint": [("self", None), ("P", None)],
    "closestElementAndBaryCoords": [("self", None), ("P", None)],
    "closestNodeAndSqDist": [("self", None), ("P", None)],
    "contains": [("self", None), ("P", None), ("eps", "1e-10")],
    "sample": [("self", None), ("P", None), ("fieldValues", None)],
}


def _arguments(doc, name):
    """[(argument name, default or None)] from the signature line pybind11 writes into the docstring"""
    line = doc.splitlines()[0]
    assert line.startswith(name + "(") and ") -> " in line, line
    inner, out, depth, cur = line[len(name) + 1:line.rindex(") -> ")], [], 0, ""
    for ch in inner + ",":
        depth += ch in "[("
        depth -= ch in "])"
        if ch == "," and depth == 0:
            out.append(cur.strip()); cur = ""
        else:
            cur += ch
    return [(a.split(":")[0].strip(), a.rsplit("=", 1)[1].strip() if "=" in a.split("]")[-1] else None) for a in out]


def check_signatures():
    for name, args in SIGNATURES.items():
        assert _arguments(getattr(cfs.FieldSampler, name).__doc__, name) == args, (name, getattr(cfs.FieldSampler, name).__doc__)
    init = cfs.FieldSampler.__init__.__doc__
    assert "(self: field_sampler.FieldSampler, mesh: " in init and ", V: " in init and ", F: " in init, init
    assert "lowest index" in cfs.__doc__


def _mesh(dim):
    if dim == 3:
        V, T = O.grid_tet_mesh(3, 2, 2)
    else:
        V, Q = O.gen_grid_2d(4, 3)
        V, T = O.quad_tri_subdiv(V, Q)
        V = V[:, :2]
    V = V + 0.08 * np.random.default_rng(3).standard_normal(V.shape)
    return np.ascontiguousarray(V), np.ascontiguousarray(T)


def _points(V, T, rng):
    e = rng.integers(0, len(T), 120)
    Pin = np.einsum("pk,pka->pa", rng.dirichlet(np.ones(T.shape[1]), 120), V[T[e]])
    Pin = Pin[R.bary_in(V, T, e, Pin).min(axis=1) > 1e-6]
    mn, mx = V.min(0), V.max(0)
    Pout = mn + (mx - mn) * rng.uniform(-0.5, 1.5, (60, V.shape[1]))
    Pout = Pout[R.locate(V, T, Pout)[0] < 0]
    return np.concatenate([Pin, Pout]), len(Pin)


def check_device():
    import meshfem_amd as M
    rng = np.random.default_rng(0)
    for dim in (2, 3):
        V, T = _mesh(dim)
        P, na = _points(V, T, rng)
        rI, rB, rC, rd2 = R.locate_full(V, T, P)
        diag2 = np.linalg.norm(V.max(0) - V.min(0)) ** 2
        for deg in (1, 2):
            c = M.Context(0)                         # the node numbering of the library, for the restatement
            c.mesh_build(T, V, deg)
            en, npos = c.elem_nodes(), c.node_positions()
            c.close()
            for fs, raw in ((cfs.FieldSampler(cmesh.Mesh(V, T, deg, dim)), False), (cfs.FieldSampler(V, T), True)):
                if raw and deg == 2:
                    continue
                I, Cl = fs.closestElementAndPoint(P)
                I2, B = fs.closestElementAndBaryCoords(P)
                assert I.dtype == np.int32 and np.array_equal(I, I2) and Cl.shape == P.shape and B.shape == (len(P), dim + 1)
                assert np.array_equal(I[:na], rI[:na]) and np.abs(B[:na] - rB[:na]).max() <= 1e-10 and np.array_equal(Cl[:na], P[:na])
                assert np.abs(Cl - rC).max() <= 1e-12 * diag2
                assert np.all(np.sqrt(R.dist2_to_elements(V, T, I[na:], P[na:])) - np.sqrt(rd2[na:]) <= 1e-12 * np.sqrt(diag2))
                inside = fs.contains(P)
                assert inside.dtype == np.bool_ and np.array_equal(inside, rd2 <= 1e-20)
                assert fs.contains(P, eps=1e3).all() and np.array_equal(fs.contains(P, 1e-10), inside)
                # the three kinds of field, with and without a component axis
                lin = lambda X: np.stack([1.0 + X @ np.arange(1.0, dim + 1), X[:, 0] - 2.0 * X[:, dim - 1], 0.5 - X[:, 1]], axis=1)
                sv = fs.sample(P, lin(V))
                assert sv.shape == (len(P), 3) and np.abs(sv - lin(Cl)).max() <= 1e-12 * np.abs(lin(V)).max()
                assert np.array_equal(fs.sample(P, lin(V)[:, 0]), sv[:, 0])
                fe = rng.standard_normal((len(T), 2))
                assert np.array_equal(fs.sample(P, fe), fe[I])
                if raw:
                    try:
                        fs.closestNodeAndSqDist(P)
                        raise AssertionError("a raw mesh must raise")
                    except RuntimeError as ex:
                        assert "Unsupported for raw meshes" in str(ex)
                    continue
                quad = lambda X: np.stack([lin(X)[:, 0] + (X[:, 0] * X[:, 1] if deg == 2 else 0.0), lin(X)[:, 1] - (X[:, dim - 1] ** 2 if deg == 2 else 0.0)], axis=1)
                f = quad(npos)
                if len(npos) != len(V) and len(npos) != len(T):
                    sn = fs.sample(P, f)
                    assert np.abs(sn - quad(Cl)).max() <= 1e-12 * np.abs(f).max()
                    assert np.abs(sn - R.sample(en, len(V), deg, I, B, f)).max() <= 1e-12 * np.abs(f).max()
                NI, nd2 = fs.closestNodeAndSqDist(P)
                rnode, rnd2, lead = R.closest_node(en, npos, deg, rI, rB, P)
                ok = lead > 1e-9
                ok[na:] &= I[na:] == rI[na:]
                assert NI.dtype == np.int32 and ok[:na].mean() >= 0.9
                assert np.array_equal(NI[ok], rnode[ok]) and np.abs(nd2[ok] - rnd2[ok]).max() <= 1e-12 * diag2
                try:
                    fs.sample(P, np.zeros((len(npos) + len(T) + 1, 2)))
                    raise AssertionError("a field of the wrong size must raise")
                except RuntimeError as ex:
                    assert "Invalid fieldValues size" in str(ex)
    # triangles embedded in 3D are refused with a clear message
    V, T = _mesh(2)
    V3 = np.concatenate([V, np.zeros((len(V), 1))], axis=1)
    try:
        cfs.FieldSampler(V3, T)
        raise AssertionError("triangles in 3D must raise")
    except RuntimeError as ex:
        assert "embedded in 3D" in str(ex)


if __name__ == "__main__":
    check_signatures()
    if sys.argv[1:] == ["gpu"]:
        check_device()
    print("ok")
