"""The field sampler on the device (mfh_locate, mfh_sample_field, mfh_closest_node, mfh_sampler_build / _info; meshfem_amd/csrc/mfh_sampler.hip)
against the brute-force numpy restatement (tests/field_sampler_util.py): every point against every element, no spatial index.

Bounds. Barycentric coordinates of contained points: 1e-10. Closest points and squared distances of outside points: 1e-12 of the squared
bounding-box diagonal. Sampled polynomials: 1e-12 max|q|. Shared points (vertices, edge midpoints, centroids): the returned element must hold
the point (brute-force min lambda >= -1e-12), and it must be the brute-force lowest index whenever no element's brute-force min lambda lies
within MARGIN of the threshold -1e-12. MARGIN is 1e-13, not 1e-9: a point ON a shared vertex or edge has min lambda = 0 up to a few 1e-16 in
every element around it, i.e. 1e-12 from the threshold, so a margin of 1e-9 would put every shared point into the "only validity" class and
the 90 % that the same specification wants in the strict class could not be met; the smaller margin asks for index equality at MORE points.
It still exceeds what the two evaluations of lambda can differ by (a few eps times |grad lambda| |p - x0| < 1e-14 on these meshes).
The per-point kernels cap their grids at 4096 workgroups of 256 lanes, the build kernels at 1024."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import field_sampler_util as R
import test_gpu_stress_measures as S

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

CASES = [(2, 1), (2, 2), (3, 1), (3, 2)]
SCALES = [0.25, 1.0, 1e6]
MARGIN = 1e-13
POINT_CAP, BUILD_CAP = 4096 * 256, 1024 * 256


def _mesh(dim, notch):
    V, T = S._mesh(dim)
    if notch:                           # one corner block of the grid (4 x 3 quads / 3 x 2 x 2 cubes of edge 1) removed
        cen = V[T].mean(axis=1)
        lo = np.array([3.0, 2.0] if dim == 2 else [2.0, 1.0, 1.0])
        T = T[~np.all(cen > lo, axis=1)]
        used = np.unique(T)
        renum = np.full(len(V), -1)
        renum[used] = np.arange(len(used))
        V, T = V[used], renum[T]
    return np.ascontiguousarray(V), np.ascontiguousarray(T)


def _queries(dim, V, T, notch, rng):
    """sets (a) interior, (b) shared points, (c) outside (without the far points), as arrays"""
    nv = dim + 1
    e = rng.integers(0, len(T), 400)
    Pa = np.einsum("pk,pka->pa", rng.dirichlet(np.ones(nv), 400), V[T[e]])
    keep = R.bary_in(V, T, e, Pa).min(axis=1) > 1e-6
    Pa = Pa[keep]
    edges = np.unique(np.sort(np.concatenate([T[:, [i, j]] for i in range(nv) for j in range(i + 1, nv)]), axis=1), axis=0)
    shared = [V, V[edges].mean(axis=1), V[T].mean(axis=1)]
    if dim == 3:
        faces = np.unique(np.sort(np.concatenate([np.delete(T, k, axis=1) for k in range(4)]), axis=1), axis=0)
        shared.append(V[faces].mean(axis=1))
    Pb = np.concatenate(shared)
    mn, mx = V.min(0), V.max(0)
    diag = np.linalg.norm(mx - mn)
    n = 160
    Pc = mn + (mx - mn) * rng.uniform(-0.5, 1.5, (n, dim))            # around the box: beyond faces, edges and corners of it
    axis, side = rng.integers(0, dim, n), rng.integers(0, 2, n)
    dist = diag * 10.0 ** rng.uniform(-2, np.log10(2.0), n)            # 0.01 to 2 diagonals
    Pc[np.arange(n), axis] = np.where(side == 1, mx[axis] + dist, mn[axis] - dist)
    corners = np.where(rng.integers(0, 2, (40, dim)) == 1, mx, mn)
    Pcorner = corners + np.sign(corners - 0.5 * (mn + mx)) * diag * 10.0 ** rng.uniform(-2, 0.3, (40, dim))
    out = [Pc, Pcorner]
    if notch:
        lo = np.array([3.0, 2.0] if dim == 2 else [2.0, 1.0, 1.0])
        Pn = lo + (mx - lo) * rng.uniform(0.0, 1.0, (80, dim))
        out.append(Pn[R.locate(V, T, Pn)[0] < 0])
    Pc = np.concatenate(out)
    assert np.all(R.locate(V, T, Pc)[0] < 0)
    return Pa, Pb, Pc


@functools.lru_cache(maxsize=None)
def _case(dim, deg, notch=False):
    """context, mesh, node tables, query sets and the brute-force answers: computed once, read by every test"""
    import meshfem_amd as M
    V, T = _mesh(dim, notch)
    c = M.Context(0)
    c.mesh_build(T, V, deg)
    rng = np.random.default_rng(100 * dim + 10 * deg + int(notch))
    Pa, Pb, Pc = _queries(dim, V, T, notch, rng)
    d = dict(c=c, deg=deg, notch=notch, V=V, T=T, en=c.elem_nodes(), npos=c.node_positions(), Pa=Pa, Pb=Pb, Pc=Pc, diag=np.linalg.norm(V.max(0) - V.min(0)))
    d["P"] = np.concatenate([Pa, Pb, Pc])
    d["ref"] = R.locate_full(V, T, d["P"])
    d["mn"] = R.locate(V, T, d["P"])[2]
    for a in list(d.values()) + list(d["ref"]):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@contextlib.contextmanager
def _cell_scale(c, scale):
    """sampler_cell_scale on a cached context, put back whatever the body does"""
    c.set_option("sampler_cell_scale", scale)
    try:
        yield
    finally:
        c.set_option("sampler_cell_scale", 1.0)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("notch", [False, True])
@pytest.mark.parametrize("dim,deg", CASES)
def test_locate_against_brute_force(dim, deg, notch, scale):
    k = _case(dim, deg, notch)
    c, V, T, diag = k["c"], k["V"], k["T"], k["diag"]
    with _cell_scale(c, scale):
        _locate_checks(k, scale)


def _locate_checks(k, scale):
    c, V, T, diag = k["c"], k["V"], k["T"], k["diag"]
    dim, deg, notch = V.shape[1], k["deg"], k["notch"]
    na, nb = len(k["Pa"]), len(k["Pb"])
    I, B, Cl, d2 = c.locate(k["P"])
    rI, rB, rC, rd2 = k["ref"]
    info = c.sampler_info()
    print("%dD P%d notch=%d scale %g: %s" % (dim, deg, notch, scale, info))
    assert info["elements"]["built"] and info["boundary"]["built"] and info["elements"]["items"] == len(T)
    if scale == 1e6:
        assert info["elements"]["cells"] == [1, 1, 1] and info["elements"]["pairs"] == len(T) == info["elements"]["max_cell_population"]
    if scale == 0.25:
        assert info["elements"]["pairs"] > 2 * len(T) and info["elements"]["pairs"] <= 32 * len(T)
    # (a) strictly interior
    a = slice(0, na)
    print("  (a) %d points: max |B - ref| %.2e" % (na, np.abs(B[a] - rB[a]).max()))
    assert np.array_equal(I[a], rI[a])
    assert np.abs(B[a] - rB[a]).max() <= 1e-10
    assert np.all(d2[a] == 0) and np.array_equal(Cl[a], k["P"][a])
    # (b) shared points
    b = np.arange(na, na + nb)
    mnb = k["mn"][b]
    assert np.all(I[b] >= 0)
    chosen = mnb[np.arange(nb), I[b]]
    assert np.all(chosen >= -R.CONTAIN_TOL)
    strict = np.all(np.abs(mnb + R.CONTAIN_TOL) > MARGIN, axis=1)
    print("  (b) %d points, %d in the strict class, lowest min lambda of a returned element %.2e" % (nb, strict.sum(), chosen.min()))
    assert strict.mean() >= 0.9
    assert np.array_equal(I[b][strict], rI[b][strict])
    assert np.all(d2[b] == 0) and np.array_equal(Cl[b], k["P"][b])
    assert np.abs(np.einsum("pk,pka->pa", B[b], V[T[I[b]]]) - k["P"][b]).max() <= 1e-10
    # (c) outside
    o = np.arange(na + nb, len(k["P"]))
    eC, ed = np.abs(Cl[o] - rC[o]).max(), np.abs(d2[o] - rd2[o]).max()
    print("  (c) %d points: max |C - ref| %.2e, max |sqDist - ref| %.2e (bound %.2e)" % (len(o), eC, ed, 1e-12 * diag ** 2))
    assert eC <= 1e-12 * diag ** 2 and ed <= 1e-12 * diag ** 2
    assert np.all(I[o] >= 0)
    to_elem = np.sqrt(R.dist2_to_elements(V, T, I[o], k["P"][o]))
    assert np.all(to_elem - np.sqrt(rd2[o]) <= 1e-12 * diag)
    assert np.abs(np.einsum("pk,pka->pa", B[o], V[T[I[o]]]) - Cl[o]).max() <= 1e-10
    # contains on (a) and (c)
    ac = np.concatenate([np.arange(na), o])
    assert np.array_equal(c.contains(k["P"][ac]), rd2[ac] <= 1e-20)
    assert c.contains(k["P"][:na]).all() and not c.contains(k["P"][o]).any()
    # the same call again: the same bits
    again = c.locate(k["P"])
    for x, y in zip((I, B, Cl, d2), again):
        assert np.array_equal(x, y)


def _poly(dim, deg, ncomp, rng):
    nterm = 1 + dim + (dim * (dim + 1) // 2 if deg == 2 else 0)
    coef = rng.standard_normal((nterm, ncomp))

    def q(Y):
        t = [np.ones(len(Y))] + [Y[:, a] for a in range(dim)]
        if deg == 2:
            t += [Y[:, a] * Y[:, b] for a in range(dim) for b in range(a, dim)]
        return np.stack(t, axis=1) @ coef
    return q


@pytest.mark.parametrize("ncomp", [1, 3, 7])
@pytest.mark.parametrize("dim,deg", CASES)
def test_sample_reproduces_polynomials(dim, deg, ncomp):
    k = _case(dim, deg)
    c, V, P = k["c"], k["V"], k["P"]
    rng = np.random.default_rng(7 * ncomp + dim)
    I, B, Cl, _ = c.locate(P)
    where = Cl                                                   # inside points: p itself; outside points: the closest point of the mesh
    q = _poly(dim, deg, ncomp, rng)                              # per node: the degree of the elements
    f = q(k["npos"])
    got = c.sample(P, f)
    assert got.shape == (len(P), ncomp)
    err = np.abs(got - q(where)).max() / np.abs(f).max()
    q1 = _poly(dim, 1, ncomp, rng)                               # per vertex: linear
    fv = q1(V)
    err_v = np.abs(c.sample(P, fv) - q1(where)).max() / np.abs(fv).max()
    print("%dD P%d nComp %d: per node %.2e, per vertex %.2e" % (dim, deg, ncomp, err, err_v))
    assert err <= 1e-12 and err_v <= 1e-12
    fe = rng.standard_normal((len(k["T"]), ncomp))
    assert np.array_equal(c.sample(P, fe), fe[I])
    # against the restatement at the device's own (I, B), and the same bits twice
    assert np.abs(got - R.sample(k["en"], len(V), deg, I, B, f)).max() <= 1e-12 * np.abs(f).max()
    assert np.array_equal(c.sample(P, f), got)
    if ncomp == 1:
        assert np.array_equal(c.sample(P, f[:, 0]), got[:, 0])   # a field without a component axis


@pytest.mark.parametrize("dim,deg", CASES)
def test_closest_node(dim, deg):
    k = _case(dim, deg)
    c, P = k["c"], k["P"]
    na = len(k["Pa"])
    rI, rB = k["ref"][0], k["ref"][1]
    node, d2 = c.closest_node(P)
    rnode, rd2, lead = R.closest_node(k["en"], k["npos"], deg, rI, rB, P)
    clear = lead > 1e-9
    clear[na:na + len(k["Pb"])] = False                          # shared points: the element itself is a matter of the tie rule
    print("%dD P%d: %d of %d interior points with a clear lead" % (dim, deg, clear[:na].sum(), na))
    assert clear[:na].mean() >= 0.9
    assert np.array_equal(node[clear], rnode[clear])
    assert np.abs(d2[clear] - rd2[clear]).max() <= 1e-12 * k["diag"] ** 2
    again = c.closest_node(P)
    assert np.array_equal(node, again[0]) and np.array_equal(d2, again[1])


@pytest.mark.parametrize("dim", [2, 3])
def test_nan_empty_and_far_points(dim):
    k = _case(dim, 2)
    c, V = k["c"], k["V"]
    bad = np.tile(V.mean(0), (3, 1))
    bad[0, 0], bad[1, dim - 1], bad[2, 0] = np.nan, np.nan, np.inf
    P = np.concatenate([k["Pa"][:2], bad, k["Pc"][:2]])
    I, B, Cl, d2 = c.locate(P)
    assert np.all(I[2:5] == -1) and np.all(np.isnan(B[2:5])) and np.all(np.isnan(Cl[2:5])) and np.all(np.isnan(d2[2:5]))
    assert np.all(I[[0, 1, 5, 6]] >= 0) and not np.isnan(B[[0, 1, 5, 6]]).any()
    f = np.ones((c.n_node, 2))
    out = c.sample(P, f)
    assert np.all(np.isnan(out[2:5])) and np.abs(out[[0, 1, 5, 6]] - 1.0).max() <= 1e-12
    node, nd2 = c.closest_node(P)
    assert np.all(node[2:5] == -1) and np.all(np.isnan(nd2[2:5])) and np.all(node[[0, 1, 5, 6]] >= 0)
    assert not c.contains(P)[2:5].any()
    # nP = 0
    E = np.empty((0, dim))
    I0, B0, C0, d0 = c.locate(E)
    assert I0.shape == (0,) and B0.shape == (0, dim + 1) and C0.shape == (0, dim) and d0.shape == (0,)
    assert c.lib.mfh_sample_field(c.h, 0, None, 2, None, 1, None, 0) == 0          # nP = 0: no array is needed
    assert c.sample(E, f).shape == (0, 2) and c.closest_node(E)[0].shape == (0,) and c.contains(E).shape == (0,)
    # ten points 10^6 diagonals away: they return, with an element
    rng = np.random.default_rng(9)
    u = rng.standard_normal((10, dim))
    far = V.mean(0) + 1e6 * k["diag"] * u / np.linalg.norm(u, axis=1, keepdims=True)
    for scale in SCALES:
        with _cell_scale(c, scale):
            If, Bf, Cf, df = c.locate(far)
            assert np.all(If >= 0) and np.all(np.isfinite(df)) and np.all(df > 0)
            assert np.all(Cf >= V.min(0) - 1e-9) and np.all(Cf <= V.max(0) + 1e-9)


def _down(c, p, shape, dtype):
    from meshfem_amd._lib import ptr
    out = np.empty(shape, dtype=dtype)
    if out.nbytes:
        c.dev_memcpy(ptr(out), p, out.nbytes, 1)
    return out


@pytest.mark.parametrize("dim,deg", [(2, 2), (3, 1), (3, 2)])
def test_on_device_pointers(dim, deg):
    import meshfem_amd as M
    L = M._lib
    k = _case(dim, deg)
    c, P = k["c"], k["P"]
    n = len(P)
    f = np.random.default_rng(3).standard_normal((c.n_node, 3))
    d = S._Dev(c)
    try:
        dP, df = d.up(P), d.up(f)
        pI, pB, pC, pd = d.alloc(4 * n), d.alloc(8 * n * (dim + 1)), d.alloc(8 * n * dim), d.alloc(8 * n)
        c._ck(c.lib.mfh_locate(c.h, n, dP, pI, pB, pC, pd, 1))
        I, B, Cl, d2 = c.locate(P)
        assert np.array_equal(_down(c, pI, n, np.int32), I) and np.array_equal(_down(c, pB, B.shape, np.float64), B)
        assert np.array_equal(_down(c, pC, Cl.shape, np.float64), Cl) and np.array_equal(_down(c, pd, n, np.float64), d2)
        pd2 = d.alloc(8 * n)                                      # any output may be NULL
        c._ck(c.lib.mfh_locate(c.h, n, dP, None, None, None, pd2, 1))
        assert np.array_equal(_down(c, pd2, n, np.float64), d2)
        po = d.alloc(8 * n * 3)
        c._ck(c.lib.mfh_sample_field(c.h, n, dP, L.FIELD_PER_NODE, df, 3, po, 1))
        assert np.array_equal(_down(c, po, (n, 3), np.float64), c.sample(P, f))
        pn, pnd = d.alloc(4 * n), d.alloc(8 * n)
        c._ck(c.lib.mfh_closest_node(c.h, n, dP, pn, pnd, 1))
        node, nd2 = c.closest_node(P)
        assert np.array_equal(_down(c, pn, n, np.int32), node) and np.array_equal(_down(c, pnd, n, np.float64), nd2)
    finally:
        d.free()


@pytest.mark.parametrize("dim", [2, 3])
def test_results_follow_updated_vertices(dim):
    import meshfem_amd as M
    V, T = _mesh(dim, False)
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    rng = np.random.default_rng(12)
    e = rng.integers(0, len(T), 100)
    w = rng.dirichlet(np.ones(dim + 1), 100)
    P = np.einsum("pk,pka->pa", w, V[T[e]])
    outside = V.max(0) + 0.3
    I, B, _, _ = c.locate(np.concatenate([P, outside[None]]))
    assert c.sampler_info()["elements"]["built"]
    shift = np.arange(1, dim + 1) * 10.0
    V2 = 1.5 * V + shift                                         # far from the old positions: an index that was kept would find nothing
    c.mesh_update_vertices(V2)
    assert not c.sampler_info()["elements"]["built"]
    P2 = np.concatenate([1.5 * P + shift, (1.5 * outside + shift)[None]])
    I2, B2, C2, d2 = c.locate(P2)
    rI, rB, rC, rd2 = R.locate_full(V2, T, P2)
    lam = R.bary_in(V2, T, I2[:100], P2[:100])
    assert np.all(lam.min(axis=1) >= -R.CONTAIN_TOL) and np.abs(B2[:100] - lam).max() <= 1e-10 and np.all(d2[:100] == 0)
    clear = R.bary_in(V, T, e, P).min(axis=1) > 1e-6
    assert np.array_equal(I2[:100][clear], e[clear])
    assert abs(d2[100] - rd2[100]) <= 1e-12 * np.linalg.norm(V2.max(0) - V2.min(0)) ** 2 and d2[100] > 0
    assert not c.contains(1.5 * P + shift - 100.0).any()
    c.mesh_build(T, V, 1)                                        # a new mesh drops the index too
    assert not c.sampler_info()["elements"]["built"]
    assert np.array_equal(c.locate(P)[0][clear], e[clear])
    c.close()


def test_refusals():
    import meshfem_amd as M
    from meshfem_amd._lib import ptr
    L = M._lib
    k = _case(2, 2)
    c, P = k["c"], np.ascontiguousarray(k["Pa"][:5])
    n = len(P)
    I, d2, out = np.empty(n, dtype=np.int32), np.empty(n), np.empty((n, 2))
    f = np.zeros((c.n_node, 2))
    # no mesh
    e = M.Context(0)
    assert e.lib.mfh_locate(e.h, n, ptr(P), ptr(I), None, None, None, 0) == L.ERR_STATE
    assert e.lib.mfh_sampler_build(e.h) == L.ERR_STATE
    assert e.lib.mfh_sample_field(e.h, n, ptr(P), L.FIELD_PER_NODE, ptr(f), 2, ptr(out), 0) == L.ERR_STATE
    assert e.lib.mfh_closest_node(e.h, n, ptr(P), ptr(I), ptr(d2), 0) == L.ERR_STATE
    assert e.lib.mfh_sampler_info(e.h, C.byref(L.SamplerStats())) == L.ERR_STATE
    # a matrix loaded from triplets
    e.matrix_set_upper_triplets(3, np.array([0, 1, 2]), np.array([0, 1, 2]), np.array([1.0, 2.0, 3.0]))
    assert e.lib.mfh_locate(e.h, n, ptr(P), ptr(I), None, None, None, 0) == L.ERR_STATE
    assert e.lib.mfh_sampler_build(e.h) == L.ERR_STATE
    e.close()
    # a row-partitioned context
    V, T = _mesh(2, False)
    p = M.Context(0)
    p.mesh_set(2, 1, T, V, n_owned=len(V) - 3)
    assert p.lib.mfh_locate(p.h, n, ptr(P), ptr(I), None, None, None, 0) == L.ERR_UNSUPPORTED
    assert p.lib.mfh_sampler_build(p.h) == L.ERR_UNSUPPORTED
    assert p.lib.mfh_closest_node(p.h, n, ptr(P), ptr(I), ptr(d2), 0) == L.ERR_UNSUPPORTED
    p.close()
    # bad kind, nComp = 0, NULL P with nP > 0
    assert c.lib.mfh_sample_field(c.h, n, ptr(P), 3, ptr(f), 2, ptr(out), 0) == L.ERR_INVALID
    assert c.lib.mfh_sample_field(c.h, n, ptr(P), -1, ptr(f), 2, ptr(out), 0) == L.ERR_INVALID
    assert c.lib.mfh_sample_field(c.h, n, ptr(P), L.FIELD_PER_NODE, ptr(f), 0, ptr(out), 0) == L.ERR_INVALID
    assert c.lib.mfh_locate(c.h, n, None, ptr(I), None, None, None, 0) == L.ERR_INVALID
    assert c.lib.mfh_sample_field(c.h, n, None, L.FIELD_PER_NODE, ptr(f), 2, ptr(out), 0) == L.ERR_INVALID
    assert c.lib.mfh_closest_node(c.h, n, None, ptr(I), ptr(d2), 0) == L.ERR_INVALID
    with pytest.raises(ValueError):
        c.sample(P, np.zeros((c.n_node + 1, 2)))
    with pytest.raises(M.MeshFEMHipError):
        c.set_option("sampler_cell_scale", 0.0)
    assert c.lib.mfh_locate(c.h, n, ptr(P), ptr(I), None, None, None, 0) == L.OK       # and the context still works
    assert np.array_equal(I, k["ref"][0][:5])


def test_mesh_without_boundary_elements():
    """a mesh from mfh_mesh_set (the caller's node table) has no boundary elements: contained points are located, the others get -1 and NaN"""
    import meshfem_amd as M
    V, T = _mesh(2, False)
    c = M.Context(0)
    c.mesh_set(2, 1, T, V)
    k = _case(2, 1)
    P = np.concatenate([k["Pa"][:20], k["Pc"][:5]])
    I, B, Cl, d2 = c.locate(P)
    assert np.array_equal(I[:20], k["ref"][0][:20]) and np.all(I[20:] == -1) and np.all(np.isnan(d2[20:])) and np.all(np.isnan(B[20:]))
    c.close()


def test_points_above_the_grid_cap():
    """more points than 4096 workgroups x 256 lanes on the small 2D mesh: k_locate, k_closest_boundary (launched over all points),
    k_sample_field and k_closest_node run their grid-stride branch and a last, partial stride"""
    k = _case(2, 2)
    c, V, T = k["c"], k["V"], k["T"]
    n = POINT_CAP + 77
    rng = np.random.default_rng(21)
    mn, mx = V.min(0), V.max(0)
    P = mn + (mx - mn) * rng.uniform(-0.15, 1.15, (n, 2))        # about a third of them outside
    q = _poly(2, 2, 3, rng)
    f = q(k["npos"])
    I, B, Cl, d2 = c.locate(P)
    got = c.sample(P, f)
    node, nd2 = c.closest_node(P)
    assert np.count_nonzero(d2 > 0) > n // 10 and np.count_nonzero(d2 == 0) > n // 2
    idx = np.concatenate([np.arange(0, n, 523), [POINT_CAP - 1, POINT_CAP, n - 1]])
    rI, rB, rC, rd2 = R.locate_full(V, T, P[idx])
    mnl = R.locate(V, T, P[idx])[2]
    clear = np.all(np.abs(mnl + R.CONTAIN_TOL) > MARGIN, axis=1)
    assert clear.mean() > 0.99
    clear &= (mnl >= -R.CONTAIN_TOL).any(axis=1)                # contained points: for the others the element index is not pinned, C and sqDist are
    assert clear.sum() > 1000
    assert np.array_equal(I[idx][clear], rI[clear]) and np.abs(B[idx][clear] - rB[clear]).max() <= 1e-10
    diag2 = k["diag"] ** 2
    assert np.abs(Cl[idx] - rC).max() <= 1e-12 * diag2 and np.abs(d2[idx] - rd2).max() <= 1e-12 * diag2
    assert np.abs(got[idx] - q(Cl[idx])).max() <= 1e-12 * np.abs(f).max()
    assert np.abs(got - q(Cl)).max() <= 1e-12 * np.abs(f).max()
    rnode, rnd2, lead = R.closest_node(k["en"], k["npos"], 2, rI, rB, P[idx])
    ok = clear & (lead > 1e-9)
    assert ok.sum() > 0.9 * clear.sum() and np.array_equal(node[idx][ok], rnode[ok]) and np.abs(nd2[idx][ok] - rnd2[ok]).max() <= 1e-12 * diag2
    assert np.all(node >= 0)


def test_elements_above_the_build_cap():
    """363 x 362 quads -> 262 812 linear triangles, just above the 1024 x 256 items one pass of the build kernels covers"""
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tri_mesh(363, 362, [0.0, 0.0], [1.0, 1.0])
    T = np.ascontiguousarray(T, dtype=np.int64)
    assert len(T) > BUILD_CAP
    rng = np.random.default_rng(22)
    V = V + (0.15 / 363) * rng.uniform(-1, 1, V.shape)
    c = M.Context(0)
    c.mesh_build(T, V, 1)
    c.sampler_build()
    info = c.sampler_info()
    print(info)
    assert info["elements"]["built"] and not info["boundary"]["built"]
    assert info["elements"]["items"] == len(T) and len(T) <= info["elements"]["pairs"] <= 32 * len(T)
    e = np.concatenate([rng.integers(0, len(T), 3000), [0, BUILD_CAP - 1, BUILD_CAP, len(T) - 1]])
    P = np.einsum("pk,pka->pa", rng.dirichlet(np.ones(3), len(e)), V[T[e]])
    lam = R.bary_in(V, T, e, P)
    keep = lam.min(axis=1) > 1e-6
    I, B, Cl, d2 = c.locate(P)
    assert keep.sum() > 2500
    assert np.array_equal(I[keep], e[keep]) and np.abs(B[keep] - lam[keep]).max() <= 1e-10 and np.all(d2 == 0)
    f = 2.0 + V @ np.array([1.0, -3.0])
    assert np.abs(c.sample(P, f) - (2.0 + P @ np.array([1.0, -3.0]))).max() <= 1e-12 * np.abs(f).max()
    c.close()
