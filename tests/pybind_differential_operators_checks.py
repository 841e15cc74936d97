"""Checks of the compiled `differential_operators` module (meshfem_amd/pybind), run as a script in its own interpreter by
tests/test_pybind_differential_operators.py.
    python tests/pybind_differential_operators_checks.py cpu | gpu"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import meshfem_amd.pybind as pb                      # noqa: E402
from meshfem_amd.pybind import build as pbuild       # noqa: E402

pbuild.build(verbose=False)
sys.path.insert(0, pb.PATH)
import mesh as cmesh                                 # noqa: E402
import sparse_matrices as csm                        # noqa: E402
import differential_operators as cdo                 # noqa: E402
from oracle import meshfem_oracle as O               # noqa: E402

assert cdo.__file__.endswith(".so") and os.path.dirname(cdo.__file__) == pb.PATH, cdo.__file__

# argument names and defaults of the reference's module (src/python_bindings/differential_operators.cc)
SIGNATURES = {
    "laplacian": [("mesh", None), ("forceP1", "False"), ("upperTriOnly", "False")],
    "mass": [("mesh", None), ("lumped", "False"), ("forceP1", "False"), ("upperTriOnly", "False")],
    "mass_elasticity": [("mesh", None), ("lumped", "False"), ("forceP1", "False"), ("upperTriOnly", "False")],
    "gradient": [("mesh", None), ("scalarField", None)],
    "divergence": [("mesh", None), ("vectorField", None)],
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
        assert _arguments(getattr(cdo, name).__doc__, name) == args, (name, getattr(cdo, name).__doc__)
    assert not hasattr(cdo, "bilaplacian") and "bilaplacian" in cdo.__doc__


def _mesh(dim, deg):
    if dim == 3:
        V, T = O.grid_tet_mesh(3, 2, 2)
    else:
        V, Q = O.gen_grid_2d(4, 3)
        V, T = O.quad_tri_subdiv(V, Q)
        V = V[:, :2]
    V = V + 0.08 * np.random.default_rng(3).standard_normal(V.shape)
    return O.FEMMesh(T, V, deg), cmesh.Mesh(V, T, deg, dim)


def _dense(A):
    i, j, v = A.arrays()
    D = np.zeros((A.m, A.n))
    np.add.at(D, (i, j), v)
    return D, i, j


def _expand(s, N):
    i = (N * s.i[:, None] + np.arange(N)[None, :]).reshape(-1)
    j = (N * s.j[:, None] + np.arange(N)[None, :]).reshape(-1)
    return O.TripletMatrix.from_arrays(N * s.m, N * s.n, i, j, np.repeat(s.v, N))


def check_device():
    rng = np.random.default_rng(0)
    for dim in (2, 3):
        for deg in (1, 2):
            om, cm = _mesh(dim, deg)
            o1 = O.FEMMesh(om.elems, om.verts, 1)
            for forceP1 in (False, True):
                ref_mesh = o1 if forceP1 else om
                refs = {"laplacian": O.laplacian_triplets(ref_mesh).sum_repeated(), "mass": O.mass_triplets(ref_mesh).sum_repeated(),
                        "mass_elasticity": _expand(O.mass_triplets(ref_mesh).sum_repeated(), dim)}
                for name, ref in refs.items():
                    U_ref = ref.to_scipy().toarray()
                    F_ref = ref.to_scipy_full_from_upper().toarray()
                    tol = 1e-13 * np.abs(F_ref).max()
                    for upper in (False, True):
                        A = getattr(cdo, name)(cm, forceP1=forceP1, upperTriOnly=upper)
                        assert isinstance(A, csm.TripletMatrix) and (A.m, A.n) == F_ref.shape
                        D, i, j = _dense(A)
                        assert np.abs(D - (U_ref if upper else F_ref)).max() < tol, (dim, deg, name, forceP1, upper)
                        assert (i <= j).all() if upper else (i > j).any()
                        assert (A.symmetry_mode == csm.SymmetryMode.UPPER_TRIANGLE) == upper
                lr = O.mass_triplets(ref_mesh, lumped=True).v
                for name, N in (("mass", 1), ("mass_elasticity", dim)):
                    A = getattr(cdo, name)(cm, lumped=True, forceP1=forceP1)
                    D, i, j = _dense(A)
                    assert np.array_equal(i, j) and np.abs(np.diag(D) - np.repeat(lr, N)).max() < 1e-14 * np.abs(lr).max()
            if deg == 1:
                s, v = rng.standard_normal(om.num_nodes), rng.standard_normal((len(om.elems), dim))
                g_ref = O.grad_u_average(om, s)
                assert np.abs(cdo.gradient(cm, s) - g_ref).max() < 1e-12 * np.abs(g_ref).max()
                vol, gl = om.embeddings_batch()
                d_ref = np.zeros(om.num_nodes)
                for e, nodes in enumerate(om.elem_nodes):
                    d_ref[nodes] += vol[e] * (v[e] @ gl[e])
                assert np.abs(cdo.divergence(cm, v) - d_ref).max() < 1e-12 * np.abs(d_ref).max()
            else:
                for fn, arg in ((cdo.gradient, np.zeros(om.num_nodes)), (cdo.divergence, np.zeros((len(om.elems), dim)))):
                    try:
                        fn(cm, arg)
                        raise AssertionError("degree 2 must raise")
                    except RuntimeError:
                        pass


if __name__ == "__main__":
    check_signatures()
    if sys.argv[1:] == ["gpu"]:
        check_device()
    print("ok")
