"""Stress measures on the device (k_sym_measures, k_stress_measures, k_vertex_average, k_peak_von_mises; include/meshfem_hip.h "stress
measures on the device") against the numpy restatement of the reference's routines (tests/stress_measures_util.py).

Tolerances. von Mises values and eigenvalues of the fields of a mesh: the project's standing bound for applications, 1e-12 max|sigma|
(tests/test_scalar_operators.py); eigenvectors: |V^T V - I|_inf <= 1e-12 and |A V - V Lambda|_inf <= 1e-12 max|A|. Single hard matrices are
compared per matrix relative to |A|_F with 1e-13: the device runs at most 16 sweeps of 3 Jacobi rotations, each a backward error of a few
eps |A|, so about 300 eps = 7e-14 |A| plus LAPACK's own few eps. Vertex averages add the same terms in the same order as the
restatement; the device may contract a product and a sum into one FMA, one rounding of eps max|f| per term, at most 48 terms around a
vertex of these meshes: inside 1e-12 max|f|. Every test above the grid caps stays under the 120 s that tests/test_gpu_element_integrals.py
states for its own."""
import ctypes as C
import functools

import numpy as np
import pytest

import element_integrals_util as U
import stress_measures_util as R

pytestmark = pytest.mark.gpu

CASES = [(2, 1), (2, 2), (3, 1), (3, 2)]
MATS = ["iso", "ortho_field", "general_field"]          # MAT_ISO, MAT_ORTHO, MAT_GENERAL instantiations of the fused kernels
TOL = 1e-12
ALL = 7                                                # MEASURE_VON_MISES | MEASURE_EIGENVALUES | MEASURE_EIGENVECTORS


def _mesh(dim, seed=3):
    """the perturbed small meshes of tests/test_gpu_differential_operators.py"""
    from oracle import meshfem_oracle as O
    if dim == 3:
        V, T = O.grid_tet_mesh(3, 2, 2)
    else:
        V, Q = O.gen_grid_2d(4, 3)
        V, T = O.quad_tri_subdiv(V, Q)
        V = V[:, :2]
    V = V + 0.08 * np.random.default_rng(seed).standard_normal(V.shape)
    return np.ascontiguousarray(V), np.ascontiguousarray(T)


@functools.lru_cache(maxsize=None)
def _case(dim, deg, mat):
    """(context, random u, the stress and strain fields of the existing entry point): computed once, read by every test"""
    import meshfem_amd as M
    V, T = _mesh(dim)
    c = M.Context(0)
    c.mesh_build(T, V, deg)
    U.material(mat, dim, len(T), seed=dim)[0](c)
    u = np.random.default_rng(10 * dim + deg).standard_normal((c.n_node, dim))
    fields = {True: c.strain_field(u, True), False: c.strain_field(u, False)}
    for f in fields.values():
        f.setflags(write=False)
    u.setflags(write=False)
    return c, u, fields


def _check_measures(sig, vm, ev, vec, tag):
    dim = R.dim_of(sig)
    A = R.unflatten(sig)
    scale = np.abs(sig).max()
    assert vm.shape == sig.shape[:-1] and ev.shape == sig.shape[:-1] + (dim,) and vec.shape == sig.shape[:-1] + (dim, dim)
    e_vm = np.abs(vm - R.von_mises(sig)).max()
    e_ev = np.abs(ev - R.eigenvalues(sig)).max()
    e_orth = np.abs(np.swapaxes(vec, -1, -2) @ vec - np.eye(dim)).max()
    e_res = np.abs(A @ vec - vec * ev[..., None, :]).max()
    print("%s: max|s| %.3e  von Mises %.2e  eigenvalues %.2e  |VtV - I| %.2e  |AV - VL| %.2e" % (tag, scale, e_vm / scale, e_ev / scale, e_orth, e_res / scale))
    assert e_vm <= TOL * scale, tag
    assert e_ev <= TOL * scale, tag
    assert np.all(np.diff(ev, axis=-1) >= 0), tag
    assert e_orth <= TOL, tag
    assert e_res <= TOL * scale, tag


@pytest.mark.parametrize("mat", MATS)
@pytest.mark.parametrize("dim,deg", CASES)
def test_fused_and_supplied_measures_match_strain_field(dim, deg, mat):
    import meshfem_amd as M
    c, u, fields = _case(dim, deg, mat)
    for stress in (True, False):
        sig = fields[stress]
        tag = "%dD P%d %s stress=%d" % (dim, deg, mat, stress)
        vm, ev, vec = c.stress_measures(u, ALL, stress)
        _check_measures(sig, vm, ev, vec, tag + " fused")
        vm2, ev2, vec2 = c.stress_measures(u, ALL, stress)
        assert np.array_equal(vm, vm2) and np.array_equal(ev, ev2) and np.array_equal(vec, vec2)
        # single measures write the same numbers as the combined call
        assert np.array_equal(c.von_mises(u, stress), vm)
        assert np.array_equal(c.principal_values(u, stress), ev)
        pe, pv = c.principal_values(u, stress, vectors=True)
        assert np.array_equal(pe, ev) and np.array_equal(pv, vec)
        # the supplied-field kernel on the array of the existing entry point
        svm, sev, svec = M.sym_measures(sig, ALL, ctx=c)
        _check_measures(sig, svm, sev, svec, tag + " supplied")
        again = M.sym_measures(sig, ALL, ctx=c)
        assert np.array_equal(svm, again[0]) and np.array_equal(sev, again[1]) and np.array_equal(svec, again[2])
        assert np.array_equal(M.von_mises(sig, ctx=c), svm) and np.array_equal(M.principal_values(sig, ctx=c), sev)


def _hard(dim, rng):
    """[(name, matrices [n, dim, dim])]"""
    I = np.eye(dim)
    Q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    out = [("zero", np.zeros((1, dim, dim))), ("c I", np.stack([2.5 * I, -1e-3 * I]))]
    if dim == 3:
        out.append(("two equal eigenvalues", np.stack([Q @ np.diag([2.0, 2.0, -1.0]) @ Q.T, Q @ np.diag([-3.0, 0.5, 0.5]) @ Q.T, np.diag([1.0, 4.0, 4.0])])))
    else:
        out.append(("two equal eigenvalues", np.stack([Q @ np.diag([2.0, 2.0]) @ Q.T, np.diag([-0.5, -0.5])])))
    out.append(("diagonal", np.stack([np.diag(np.arange(dim, 0, -1.0)), np.diag(-np.arange(1.0, dim + 1))])))
    D = np.diag(rng.uniform(1.0, 2.0, dim))
    off = rng.standard_normal((dim, dim))
    out.append(("tiny off-diagonals", (D + 1e-20 * (off + off.T - 2 * np.diag(np.diag(off))))[None]))
    B = rng.standard_normal((4, dim, dim))
    B = B + np.swapaxes(B, 1, 2)
    out.append(("1e150", 1e150 * B))
    out.append(("1e-150", 1e-150 * B))
    G = rng.standard_normal((3, dim, dim))
    out.append(("negative definite", -(G @ np.swapaxes(G, 1, 2) + 0.1 * I)))
    S = rng.standard_normal((3000, dim, dim)) * 10.0 ** rng.uniform(-3, 3, (3000, 1, 1))
    out.append(("random", S + np.swapaxes(S, 1, 2)))
    return out


@pytest.mark.parametrize("dim", [2, 3])
def test_hard_tensors(dim):
    import meshfem_amd as M
    c = M.Context(0)                                    # no mesh: the supplied-field kernel needs a device and a stream only
    for name, A in _hard(dim, np.random.default_rng(40 + dim)):
        f = R.flatten(A)
        vm, ev, vec = M.sym_measures(f, ALL, ctx=c)
        nrm = np.sqrt((A * A).sum(axis=(1, 2)))
        ref = np.linalg.eigvalsh(A)
        assert np.all(np.isfinite(vm)) and np.all(np.isfinite(ev)) and np.all(np.isfinite(vec)), name
        assert np.all(np.diff(ev, axis=1) >= 0), name
        e_ev = np.abs(ev - ref).max(axis=1)
        big = nrm.max() if nrm.max() > 0 else 1.0
        scaled = A / big                                # von Mises is homogeneous of degree 1: a reference that cannot overflow
        e_vm = np.abs(vm / big - R.von_mises(R.flatten(scaled)))
        e_res = np.abs(A @ vec - vec * ev[:, None, :]).max(axis=(1, 2))
        e_orth = np.abs(np.swapaxes(vec, 1, 2) @ vec - np.eye(dim)).max()
        pos = nrm > 0
        rel = (lambda e: float((e[pos] / nrm[pos]).max())) if pos.any() else (lambda e: float(e.max()))
        print("%dD %-22s eigenvalues %.2e |A|  von Mises %.2e |A|  |AV - VL| %.2e |A|  |VtV - I| %.2e" % (dim, name, rel(e_ev), rel(e_vm * big), rel(e_res), e_orth))
        assert np.all(e_ev <= 1e-13 * nrm), name
        assert np.all(e_vm * big <= 1e-13 * nrm), name
        assert np.all(e_res <= 1e-13 * nrm), name
        assert e_orth <= TOL, name
    c.close()


@pytest.mark.parametrize("dim,deg", CASES)
def test_vertex_average(dim, deg):
    c, u, fields = _case(dim, deg, "iso")
    fl = dim * (dim + 1) // 2
    cn, vol = c.elem_nodes()[:, :dim + 1], c.elem_volumes()
    assert cn.max() == c.n_vert - 1                     # vertex nodes come first: a vertex appears as a corner only
    rng = np.random.default_rng(50 + dim)
    for nq in (1, dim + 1):
        for ncomp in (1, dim, fl, dim * dim, 9, 11):    # 11: more than one register block of components
            f = rng.standard_normal((c.n_elem, nq, ncomp))
            got = c.vertex_averaged_field(f)
            ref = R.vertex_averaged(cn, vol, f, c.n_vert)
            err = np.abs(got - ref).max()
            print("%dD P%d nq %d C %d: %.2e max|f|" % (dim, deg, nq, ncomp, err / np.abs(f).max()))
            assert got.shape == (c.n_vert, ncomp) and err <= TOL * np.abs(f).max()
            assert np.array_equal(c.vertex_averaged_field(f), got)
        const = np.array([1.5, -2.0, 0.25, 3.0, -0.125, 7.0])[:fl]
        got = c.vertex_averaged_field(np.broadcast_to(const, (c.n_elem, nq, fl)))
        assert np.abs(got - const).max() <= 1e-14 * np.abs(const).max()
    # scalar per element, tensor-shaped trailing axes
    s = rng.standard_normal(c.n_elem)
    assert np.abs(c.vertex_averaged_field(s) - R.vertex_averaged(cn, vol, s[:, None], c.n_vert)).max() <= TOL * np.abs(s).max()
    t = rng.standard_normal((c.n_elem, dim + 1, dim, dim))
    got = c.vertex_averaged_field(t)
    assert got.shape == (c.n_vert, dim, dim) and np.abs(got - R.vertex_averaged(cn, vol, t, c.n_vert)).max() <= TOL * np.abs(t).max()
    # the convenience route keeps the corner field on the device: the same kernel on the same numbers
    for stress in (True, False):
        one = c.vertex_averaged_stress(u) if stress else c.vertex_averaged_strain(u)
        assert np.array_equal(one, c.vertex_averaged_field(fields[stress]))
        assert np.array_equal(one, c.vertex_averaged_stress(u) if stress else c.vertex_averaged_strain(u))
        assert np.abs(one - R.vertex_averaged(cn, vol, fields[stress], c.n_vert)).max() <= TOL * np.abs(fields[stress]).max()


@pytest.mark.parametrize("dim,deg", CASES)
def test_vertex_of_one_element_takes_its_value(dim, deg):
    """two elements sharing a face: the two vertices opposite to it belong to one element each"""
    import meshfem_amd as M
    rng = np.random.default_rng(60 + dim)
    if dim == 2:
        V, T = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]), np.array([[0, 1, 2], [1, 3, 2]])
    else:
        V, T = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 1, 0], [0.0, 0, 1], [1.0, 1, 1]]), np.array([[0, 1, 2, 3], [1, 2, 3, 4]])
    V = V + 0.07 * rng.standard_normal(V.shape)
    c = M.Context(0)
    c.mesh_build(T, V, deg)
    cn = c.elem_nodes()[:, :dim + 1]
    lone = np.flatnonzero(np.bincount(cn.ravel(), minlength=c.n_vert) == 1)
    assert len(lone) == 2
    for nq in (1, dim + 1):
        f = rng.standard_normal((2, nq, 5))
        got = c.vertex_averaged_field(f)
        for v in lone:
            e, k = [int(x[0]) for x in np.nonzero(cn == v)]
            assert np.array_equal(got[v], f[e, k if nq > 1 else 0])
        assert np.abs(got - R.vertex_averaged(cn, c.elem_volumes(), f, c.n_vert)).max() <= TOL * np.abs(f).max()
    c.close()


@pytest.mark.parametrize("mat", MATS)
@pytest.mark.parametrize("dim,deg", CASES)
def test_peak_is_max_and_argmax_of_the_fused_field(dim, deg, mat):
    c, u, _ = _case(dim, deg, mat)
    for stress in (True, False):
        vm = c.von_mises(u, stress)
        v, i = c.peak_von_mises(u, stress)
        assert v == vm.max() and i == int(np.argmax(vm.reshape(-1)))
        assert (v, i) == c.peak_von_mises(u, stress)
    bad = np.array(u)
    bad[c.elem_nodes()[c.n_elem // 2, 1]] = np.nan
    vm = c.von_mises(bad).reshape(-1)
    v, i = c.peak_von_mises(bad)
    assert np.isnan(vm).any() and not np.isnan(vm).all()
    assert np.isnan(v) and i == int(np.flatnonzero(np.isnan(vm))[0])


@pytest.mark.parametrize("dim,deg", CASES)
def test_peak_tie_goes_to_the_lowest_index(dim, deg):
    """Unperturbed unit cells with integer corner coordinates: every cell is an exact translate of the first one (all node coordinates
    are multiples of 1/4), and u is a table look-up in the position inside the cell, so every element has the displacements of its
    translates in the other cells, bit for bit: the maximum occurs once per cell."""
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(3, 2, 2) if dim == 3 else grid.grid_tri_mesh(4, 3)
    c = M.Context(0)
    c.mesh_build(T, V, deg)
    c.material_isotropic(200.0, 0.3)
    key = np.rint(4.0 * c.node_positions()).astype(np.int64) % 4
    table = np.random.default_rng(70 + dim).standard_normal((4,) * dim + (dim,))
    u = table[tuple(key.T)]
    vm = c.von_mises(u).reshape(-1)
    assert np.count_nonzero(vm == vm.max()) >= 2
    v, i = c.peak_von_mises(u)
    assert v == vm.max() and i == int(np.flatnonzero(vm == vm.max())[0])
    c.close()


def test_refusals():
    import meshfem_amd as M
    from meshfem_amd._lib import ptr
    L = M._lib
    c, u, fields = _case(2, 2, "iso")
    # a requested output that is null
    vm = np.empty((c.n_elem, 3))
    assert c.lib.mfh_stress_measures(c.h, ptr(u), 1, L.MEASURE_VON_MISES | L.MEASURE_EIGENVALUES, ptr(vm), None, None, 0) == L.ERR_INVALID
    assert c.lib.mfh_stress_measures(c.h, ptr(u), 1, L.MEASURE_EIGENVECTORS, ptr(vm), None, None, 0) == L.ERR_INVALID
    sig = np.ascontiguousarray(fields[True])
    assert c.lib.mfh_sym_measures(c.h, 2, sig.size // 3, ptr(sig), L.MEASURE_VON_MISES, None, None, None, 0) == L.ERR_INVALID
    assert c.lib.mfh_sym_measures(c.h, 2, sig.size // 3, ptr(sig), 0, None, None, None, 0) == L.ERR_INVALID
    # outputs that are not requested may be null
    assert c.lib.mfh_stress_measures(c.h, ptr(u), 1, L.MEASURE_VON_MISES, ptr(vm), None, None, 0) == L.OK
    # a scalar operator: no stress
    V, T = _mesh(2)
    s = M.Context(0)
    s.mesh_build(T, V, 1)
    s.set_operator(M.OP_LAPLACIAN)
    us = np.zeros((s.n_node, 2))
    for call in (lambda: s.von_mises(us, stress=True), lambda: s.principal_values(us, stress=True), lambda: s.peak_von_mises(us, stress=True),
                 lambda: s.vertex_averaged_stress(us)):
        with pytest.raises(M.MeshFEMHipError) as ei:
            call()
        assert ei.value.code == L.ERR_STATE
    s.close()
    # a row-partitioned context: the elements of other ranks are missing at the interface vertices
    p = M.Context(0)
    p.mesh_set(2, 1, T, V, n_owned=len(V) - 3)
    p.material_isotropic(200.0, 0.3)
    for call in (lambda: p.vertex_averaged_field(np.zeros((len(T), 1, 2))), lambda: p.vertex_averaged_stress(np.zeros((len(V), 2)))):
        with pytest.raises(M.MeshFEMHipError) as ei:
            call()
        assert ei.value.code == L.ERR_UNSUPPORTED
    assert p.von_mises(np.zeros((len(V), 2))).shape == (len(T), 1)          # the per-element measures need no neighbours
    p.close()


class _Dev:
    """device arrays through the library's arena, filled and read back with mfh_dev_memcpy"""

    def __init__(self, c):
        self.c, self.ptrs = c, []

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.c._ck(self.c.lib.mfh_debug_arena_alloc(self.c.h, int(nbytes), C.byref(p)))
        self.ptrs.append(p.value)
        return p.value

    def up(self, a):
        from meshfem_amd._lib import ptr
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = self.alloc(a.nbytes)
        self.c.dev_memcpy(p, ptr(a), a.nbytes, 0)
        return p

    def down(self, p, shape):
        from meshfem_amd._lib import ptr
        out = np.empty(shape)
        self.c.dev_memcpy(ptr(out), p, out.nbytes, 1)
        return out

    def free(self):
        for p in self.ptrs:
            self.c._ck(self.c.lib.mfh_debug_arena_free(self.c.h, C.c_void_p(p)))


@pytest.mark.parametrize("dim,deg", [(2, 2), (3, 2), (3, 1)])
def test_on_device_pointers(dim, deg):
    import meshfem_amd as M
    c, u, fields = _case(dim, deg, "ortho_field")
    fl, nq = dim * (dim + 1) // 2, 1 if deg == 1 else dim + 1
    n = c.n_elem * nq
    d = _Dev(c)
    try:
        du = d.up(u)
        pvm, pev, pvec = d.alloc(8 * n), d.alloc(8 * n * dim), d.alloc(8 * n * dim * dim)
        c._ck(c.lib.mfh_stress_measures(c.h, du, 1, ALL, pvm, pev, pvec, 1))
        vm, ev, vec = c.stress_measures(u, ALL, True)
        assert np.array_equal(d.down(pvm, vm.shape), vm) and np.array_equal(d.down(pev, ev.shape), ev) and np.array_equal(d.down(pvec, vec.shape), vec)
        sig = fields[True]
        dsig = d.up(sig)
        qvm, qev = d.alloc(8 * n), d.alloc(8 * n * dim)
        c._ck(c.lib.mfh_sym_measures(c.h, dim, n, dsig, 3, qvm, qev, None, 1))
        svm, sev, _ = M.sym_measures(sig, 3, ctx=c)
        assert np.array_equal(d.down(qvm, svm.shape), svm) and np.array_equal(d.down(qev, sev.shape), sev)
        pavg = d.alloc(8 * c.n_vert * fl)
        c._ck(c.lib.mfh_vertex_average(c.h, dsig, int(nq > 1), fl, pavg, 1))
        assert np.array_equal(d.down(pavg, (c.n_vert, fl)), c.vertex_averaged_field(sig))
        pavg2 = d.alloc(8 * c.n_vert * fl)
        c._ck(c.lib.mfh_vertex_averaged_strain(c.h, du, 1, pavg2, 1))
        assert np.array_equal(d.down(pavg2, (c.n_vert, fl)), c.vertex_averaged_stress(u))
    finally:
        d.free()


@pytest.mark.timeout(120)
def test_supplied_field_above_the_grid_cap():
    """launch_sym_measures caps its grid at 8192 workgroups of 256 lanes: n = 8192 x 256 + 77 runs the `+= gridDim.x * 256` branch and a
    last, partial stride."""
    import meshfem_amd as M
    n = 8192 * 256 + 77
    rng = np.random.default_rng(80)
    f = rng.standard_normal((n, 6)) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    c = M.Context(0)
    vm, ev, vec = M.sym_measures(f, ALL, ctx=c)
    idx = np.concatenate([rng.choice(n, 4000, replace=False), [0, 8192 * 256 - 1, 8192 * 256, n - 1]])
    _check_measures(f[idx], vm[idx], ev[idx], vec[idx], "above the cap, sample")
    ref_sum = R.von_mises(f).sum()
    assert abs(vm.sum() - ref_sum) <= TOL * ref_sum
    assert np.all(np.diff(ev, axis=1) >= 0)
    c.close()


@pytest.mark.timeout(120)
def test_mesh_kernels_above_the_grid_caps_2d():
    """725 x 724 quads -> 2 099 600 linear triangles (above 8192 x 256: k_stress_measures; above 1024 x 256: the first stage of the peak) on
    1 051 250 vertices (above 2048 x 256: k_vertex_average), the mesh of tests/test_gpu_element_integrals.py::test_above_the_grid_caps_2d."""
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tri_mesh(725, 724, [-0.5, -0.5], [0.5, 0.5])
    V = U.perturbed(V, 0.15 / 725)
    T = np.ascontiguousarray(T, dtype=np.int64)
    assert len(T) > 8192 * 256 and len(V) > 2048 * 256
    rng = np.random.default_rng(81)
    c = M.Context(0)
    c.mesh_build(T, V, 1)
    c.material_isotropic(200.0, 0.3)
    u = rng.standard_normal((c.n_node, 2))
    sig = c.strain_field(u, True)
    vm, ev, vec = c.stress_measures(u, ALL, True)
    idx = np.concatenate([rng.choice(len(T), 4000, replace=False), [0, 8192 * 256 - 1, 8192 * 256, len(T) - 1]])
    _check_measures(sig[idx], vm[idx], ev[idx], vec[idx], "above the cap, sampled elements")
    ref_sum = R.von_mises(sig).sum()
    assert abs(vm.sum() - ref_sum) <= TOL * ref_sum
    v, i = c.peak_von_mises(u)
    assert v == vm.max() and i == int(np.argmax(vm.reshape(-1)))
    avg = c.vertex_averaged_stress(u)
    ref = R.vertex_averaged(c.elem_nodes()[:, :3], c.elem_volumes(), sig, c.n_vert)
    vi = np.concatenate([rng.choice(c.n_vert, 4000, replace=False), [0, 2048 * 256 - 1, 2048 * 256, c.n_vert - 1]])
    assert np.abs(avg[vi] - ref[vi]).max() <= TOL * np.abs(sig).max()
    assert np.abs(avg - ref).max() <= TOL * np.abs(sig).max()
    c.close()
