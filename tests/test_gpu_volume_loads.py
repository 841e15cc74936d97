"""Volume loads on the device (k_stress_field_load, k_field_stress, k_body_force_load; include/meshfem_hip.h "volume loads") against the numpy
restatement tests/volume_loads_util.py, against identities that use only older entry points, and on closed-form solutions through Simulator.

Tolerances. Loads: the project's standing bound for applications, 1e-12 max|f_ref| (tests/test_gpu_stress_measures.py): the device adds the terms
of the restatement in the restatement's order (element order per DoF) and may contract a product and a sum into one FMA, one rounding of eps max|f|
per term, at most 48 terms around a vertex of these meshes. Solutions: the closed forms lie in the finite-element space, so the discrete solution
is the analytic one up to the solver's residual (rtol 1e-12 on systems of these sizes): 1e-9 max|u|, and 1e-9 of the stress scale for stresses
derived from them."""
import ctypes as C
import functools

import numpy as np
import pytest

import element_integrals_util as U
import volume_loads_util as R

pytestmark = pytest.mark.gpu

CASES = [(2, 1), (2, 2), (3, 1), (3, 2)]
MATS = ["iso", "ortho_field", "general_field"]
TOL = 1e-12


def _mesh(dim, seed=3):
    """the perturbed small meshes of tests/test_gpu_stress_measures.py"""
    from oracle import meshfem_oracle as O
    if dim == 3:
        V, T = O.grid_tet_mesh(3, 2, 2)
    else:
        V, Q = O.gen_grid_2d(4, 3)
        V, T = O.quad_tri_subdiv(V, Q)
        V = V[:, :2]
    V = V + 0.08 * np.random.default_rng(seed).standard_normal(V.shape)
    return np.ascontiguousarray(V), np.ascontiguousarray(T)


def _context(dim, deg, mat="iso"):
    import meshfem_amd as M
    V, T = _mesh(dim)
    c = M.Context(0)
    c.mesh_build(T, V, deg)
    D = U.material(mat, dim, len(T), seed=dim)
    D[0](c)
    return c, D[1]


@functools.lru_cache(maxsize=None)
def _case(dim, deg, mat="iso"):
    """(context, restatement, D, fields): computed once, read by every test"""
    c, D = _context(dim, deg, mat)
    r = R.Mesh(dim, deg, c.elem_nodes(), c.node_positions())
    rng = np.random.default_rng(20 * dim + deg)
    fl = dim * (dim + 1) // 2
    f = dict(sigma=rng.standard_normal((c.n_elem, fl)), eps=rng.standard_normal((c.n_elem, fl)), rho=rng.uniform(0.5, 2.0, c.n_elem),
             b=rng.standard_normal(dim), b_elem=rng.standard_normal((c.n_elem, dim)), b_node=rng.standard_normal((c.n_node, dim)),
             u=rng.standard_normal((c.n_node, dim)))
    for a in f.values():
        a.setflags(write=False)
    return c, r, D, f


def _close(got, ref, tag, tol=TOL):
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print("%s: max|ref| %.3e  error %.2e of it" % (tag, scale, err / scale))
    assert got.shape == ref.shape and err <= tol * scale, tag


# ------------------------------------------------------------------------------------------------ device against the restatement
@pytest.mark.parametrize("dim,deg", CASES)
def test_body_force_matches_the_restatement(dim, deg):
    c, r, _, f = _case(dim, deg)
    assert np.abs(c.elem_volumes() - r.vol).max() <= 1e-14 * r.vol.max()
    for name in ("b", "b_elem", "b_node"):
        for rho in (None, f["rho"]):
            got = c.body_force_load(f[name], rho)
            _close(got, r.body_force_load(f[name], rho), "%dD P%d %s density %s" % (dim, deg, name, rho is not None))
            assert np.array_equal(got, c.body_force_load(f[name], rho))


@pytest.mark.parametrize("mat", MATS)
@pytest.mark.parametrize("dim,deg", CASES)
def test_stress_field_load_matches_the_restatement(dim, deg, mat):
    c, r, D, f = _case(dim, deg, mat)
    tag = "%dD P%d %s" % (dim, deg, mat)
    got = c.stress_field_load(f["sigma"])
    _close(got, r.stress_field_load(f["sigma"]), tag + " stress kind")
    assert np.array_equal(got, c.stress_field_load(f["sigma"], "stress"))
    sig_ref = r.stress_of_strain(D, f["eps"])
    got, sig = c.stress_field_load(f["eps"], "strain", return_stress=True)
    _close(got, r.stress_field_load(sig_ref), tag + " strain kind")
    _close(sig, sig_ref, tag + " stressOut")
    assert np.array_equal(got, c.stress_field_load(f["eps"], "strain"))
    # the load of the written stress is the load of the strain (the same products in both kernels, up to contraction)
    _close(c.stress_field_load(sig), got, tag + " load of stressOut")


# ------------------------------------------------------------------------------------------------ identities on existing entry points
@pytest.mark.parametrize("mat", MATS)
@pytest.mark.parametrize("dim,deg", CASES)
def test_one_strain_everywhere_is_the_constant_strain_load(dim, deg, mat):
    c, _, _, f = _case(dim, deg, mat)
    e = np.array(f["eps"][0])
    ref = c.constant_strain_load(e)
    _close(c.stress_field_load(np.broadcast_to(e, f["eps"].shape).copy(), "strain"), ref, "%dD P%d %s" % (dim, deg, mat))


@pytest.mark.parametrize("dim,deg", CASES)
def test_work_of_the_stress_load(dim, deg):
    """f . u = sum_e vol_e sigma_e : averageStrain_e(u)"""
    c, _, _, f = _case(dim, deg)
    dbl = np.where(np.arange(f["sigma"].shape[1]) < dim, 1.0, 2.0)
    terms = c.elem_volumes()[:, None] * f["sigma"] * c.average_strain(f["u"]) * dbl
    work = float((c.stress_field_load(f["sigma"]) * f["u"]).sum())
    assert abs(work - terms.sum()) <= TOL * np.abs(terms).sum()


@pytest.mark.parametrize("dim,deg", CASES)
def test_nodal_body_force_is_the_vector_mass_matrix_times_the_field(dim, deg):
    import meshfem_amd as M
    c, _, _, f = _case(dim, deg)
    V, T = _mesh(dim)
    m = M.Context(0)
    m.mesh_build(T, V, deg)
    m.set_operator(M.OP_MASS_VECTOR)
    ref = m.apply_K(f["b_node"].reshape(-1)).reshape(-1, dim)
    m.close()
    _close(c.body_force_load(f["b_node"]), ref, "%dD P%d M b" % (dim, deg))


@pytest.mark.parametrize("dim,deg", CASES)
def test_total_of_the_constant_body_force(dim, deg):
    c, _, _, f = _case(dim, deg)
    mass = (f["rho"] * c.elem_volumes()).sum()
    total = c.body_force_load(f["b"], f["rho"]).sum(axis=0)
    # the nodal weights of a quadratic tet have both signs: the terms of the total are |w_i| mass b, sum |w_i| = 1.4
    assert np.abs(total - mass * f["b"]).max() <= TOL * 1.4 * mass * np.abs(f["b"]).max()
    if deg == 2:
        w_vertex = 0.0 if dim == 2 else -1.0 / 20.0
        one = c.body_force_load(np.eye(dim)[0])[:c.n_vert, 0]
        corners = np.bincount(c.elem_nodes()[:, :dim + 1].ravel(), weights=np.repeat(c.elem_volumes(), dim + 1), minlength=c.n_vert)
        assert np.abs(one - w_vertex * corners).max() <= TOL * corners.max()        # negative on tets, zero on triangles: as the weights are


# ------------------------------------------------------------------------------------------------ semantics
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


@pytest.mark.parametrize("dim,deg", CASES)
def test_add_flag(dim, deg):
    c, _, _, f = _case(dim, deg, "ortho_field")
    prev = np.random.default_rng(9).standard_normal((c.n_dof, dim))
    for call in (lambda **k: c.body_force_load(f["b"], f["rho"], **k), lambda **k: c.body_force_load(f["b_elem"], **k),
                 lambda **k: c.body_force_load(f["b_node"], f["rho"], **k), lambda **k: c.stress_field_load(f["sigma"], **k),
                 lambda **k: c.stress_field_load(f["eps"], "strain", **k)):
        out = prev.copy()
        assert call(out=out, add=True) is out
        assert np.array_equal(out, prev + call())
        out2 = np.full((c.n_dof, dim), np.nan)              # out-of-place writes every entry: nothing of the old content survives
        call(out=out2)
        assert np.array_equal(out2, call())


@pytest.mark.parametrize("dim,deg", [(2, 2), (3, 2), (3, 1)])
def test_on_device_pointers(dim, deg):
    from meshfem_amd import _lib as L
    from meshfem_amd._lib import ptr
    c, _, _, f = _case(dim, deg, "general_field")
    n, fl = c.n_dof * dim, dim * (dim + 1) // 2
    d = _Dev(c)
    try:
        rho, out = d.up(f["rho"]), d.alloc(8 * n)
        b = np.ascontiguousarray(f["b"])
        c._ck(c.lib.mfh_body_force_load(c.h, L.BODY_CONSTANT, ptr(b), rho, L.LOAD_ON_DEVICE, out))       # (the one vector is always a host pointer)
        assert np.array_equal(d.down(out, (c.n_dof, dim)), c.body_force_load(f["b"], f["rho"]))
        for kind, name in ((L.BODY_ELEMENT, "b_elem"), (L.BODY_NODE, "b_node")):
            c._ck(c.lib.mfh_body_force_load(c.h, kind, d.up(f[name]), rho, L.LOAD_ON_DEVICE, out))
            assert np.array_equal(d.down(out, (c.n_dof, dim)), c.body_force_load(f[name], f["rho"]))
        c._ck(c.lib.mfh_body_force_load(c.h, L.BODY_NODE, d.up(f["b_node"]), None, L.LOAD_ON_DEVICE | L.LOAD_ADD, out))
        assert np.array_equal(d.down(out, (c.n_dof, dim)), c.body_force_load(f["b_node"], f["rho"]) + c.body_force_load(f["b_node"]))
        c._ck(c.lib.mfh_stress_field_load(c.h, L.FIELD_LOAD_STRESS, d.up(f["sigma"]), None, L.LOAD_ON_DEVICE, out))
        assert np.array_equal(d.down(out, (c.n_dof, dim)), c.stress_field_load(f["sigma"]))
        sig = d.alloc(8 * c.n_elem * fl)
        c._ck(c.lib.mfh_stress_field_load(c.h, L.FIELD_LOAD_STRAIN, d.up(f["eps"]), sig, L.LOAD_ON_DEVICE, out))
        load, s = c.stress_field_load(f["eps"], "strain", return_stress=True)
        assert np.array_equal(d.down(out, (c.n_dof, dim)), load) and np.array_equal(d.down(sig, (c.n_elem, fl)), s)
        # the density check of a device array runs on the device
        bad = np.array(f["rho"])
        bad[c.n_elem // 2] = -1.0
        assert c.lib.mfh_body_force_load(c.h, L.BODY_CONSTANT, ptr(b), d.up(bad), L.LOAD_ON_DEVICE, out) == L.ERR_INVALID
        assert np.array_equal(d.down(out, (c.n_dof, dim)), load)                                          # nothing was written
    finally:
        d.free()


@pytest.mark.parametrize("dim,deg", CASES)
def test_fresh_context_gives_the_same_bits(dim, deg):
    c, _, _, f = _case(dim, deg, "ortho_field")
    c2, _ = _context(dim, deg, "ortho_field")
    assert np.array_equal(c2.body_force_load(f["b_node"], f["rho"]), c.body_force_load(f["b_node"], f["rho"]))
    assert np.array_equal(c2.body_force_load(f["b"], f["rho"]), c.body_force_load(f["b"], f["rho"]))
    assert np.array_equal(c2.stress_field_load(f["eps"], "strain"), c.stress_field_load(f["eps"], "strain"))
    c2.close()


@pytest.mark.parametrize("dim,deg", CASES)
def test_periodic_dof_map_sums_the_images(dim, deg):
    """the unit cell with its interior perturbed: the load under the periodic DoF map is P^T (the load per node), every DoF adding its images in
    a fixed order; removing the conditions brings the per-node load back"""
    from meshfem_amd import grid
    from meshfem_amd.linear_elasticity import Simulator
    V, T = grid.grid_tet_mesh(3, 2, 2, [0, 0, 0], [1, 1, 1]) if dim == 3 else grid.grid_tri_mesh(4, 3, [0, 0], [1, 1])
    V = U.perturbed(V, 0.05)
    sim = Simulator(T, V, deg)
    sim.setIsotropicMaterial(200.0, 0.3)
    c = sim.ctx
    rng = np.random.default_rng(31 + dim)
    sigma, b_node, rho = rng.standard_normal((c.n_elem, dim * (dim + 1) // 2)), rng.standard_normal((c.n_node, dim)), rng.uniform(0.5, 2.0, c.n_elem)
    calls = (lambda: sim.perElementStressFieldLoad(sigma), lambda: sim.perElementStrainFieldLoad(sigma), lambda: sim.bodyForceLoad(b_node, rho),
             lambda: sim.gravityLoad(np.arange(1.0, dim + 1), rho))
    per_node = [call() for call in calls]
    n_dof = sim.applyPeriodicConditions()
    assert n_dof < c.n_node and c.n_dof == n_dof
    dof, _ = c.get_dof_map()
    for call, fn in zip(calls, per_node):
        ref = np.zeros((n_dof, dim))
        np.add.at(ref, dof, fn)
        got = call()
        _close(got, ref, "%dD P%d periodic" % (dim, deg))
        assert np.array_equal(got, call())
    sim.removePeriodicConditions()
    for call, fn in zip(calls, per_node):
        assert np.array_equal(call(), fn)
    c.close()


def test_python_layer_refuses_bad_shapes():
    c, _, _, f = _case(2, 1)
    for bad in (np.zeros(3), np.zeros((c.n_elem + 1, 2)), np.zeros((c.n_node, 3))):
        with pytest.raises(ValueError):
            c.body_force_load(bad)
    with pytest.raises(ValueError):
        c.body_force_load(f["b"], np.ones(c.n_elem + 1))
    with pytest.raises(ValueError):
        c.stress_field_load(f["sigma"], "stress", return_stress=True)
    with pytest.raises(ValueError):
        c.body_force_load(f["b"], add=True)


def test_error_codes():
    import meshfem_amd as M
    from meshfem_amd import _lib as L
    from meshfem_amd._lib import ptr
    c, r, _, f = _case(2, 2)
    lib = c.lib
    out, sig = np.empty((c.n_dof, 2)), np.empty((c.n_elem, 3))
    b, be, s, rho = (np.ascontiguousarray(f[k]) for k in ("b", "b_elem", "sigma", "rho"))
    # MFH_ERR_INVALID: unknown kind, a null array that is needed, stressOut with the STRESS kind, a bad density entry
    assert lib.mfh_body_force_load(c.h, 3, ptr(b), None, 0, ptr(out)) == L.ERR_INVALID
    assert lib.mfh_body_force_load(c.h, -1, ptr(b), None, 0, ptr(out)) == L.ERR_INVALID
    assert lib.mfh_body_force_load(c.h, L.BODY_ELEMENT, None, None, 0, ptr(out)) == L.ERR_INVALID
    assert lib.mfh_body_force_load(c.h, L.BODY_CONSTANT, ptr(b), None, 0, None) == L.ERR_INVALID
    assert lib.mfh_stress_field_load(c.h, 2, ptr(s), None, 0, ptr(out)) == L.ERR_INVALID
    assert lib.mfh_stress_field_load(c.h, L.FIELD_LOAD_STRESS, None, None, 0, ptr(out)) == L.ERR_INVALID
    assert lib.mfh_stress_field_load(c.h, L.FIELD_LOAD_STRAIN, ptr(s), None, 0, None) == L.ERR_INVALID
    assert lib.mfh_stress_field_load(c.h, L.FIELD_LOAD_STRESS, ptr(s), ptr(sig), 0, ptr(out)) == L.ERR_INVALID
    for v in (-1e-300, -1.0, np.nan, np.inf, -np.inf):
        bad = rho.copy()
        bad[c.n_elem - 1] = v
        out[:] = 7.0
        assert lib.mfh_body_force_load(c.h, L.BODY_ELEMENT, ptr(be), ptr(bad), 0, ptr(out)) == L.ERR_INVALID, v
        assert np.all(out == 7.0)
    zero = rho.copy()
    zero[0] = 0.0                                           # a void element is a density, not an error
    assert lib.mfh_body_force_load(c.h, L.BODY_ELEMENT, ptr(be), ptr(zero), 0, ptr(out)) == L.OK
    # MFH_ERR_STATE: no mesh; a matrix from mfh_matrix_set_upper_triplets
    e = M.Context(0)
    assert e.lib.mfh_body_force_load(e.h, L.BODY_CONSTANT, ptr(b), None, 0, ptr(out)) == L.ERR_STATE
    assert e.lib.mfh_stress_field_load(e.h, L.FIELD_LOAD_STRESS, ptr(s), None, 0, ptr(out)) == L.ERR_STATE
    e.matrix_set_upper_triplets(3, [0, 1, 2], [0, 1, 2], [1.0, 2.0, 3.0])
    assert e.lib.mfh_body_force_load(e.h, L.BODY_CONSTANT, ptr(b), None, 0, ptr(out)) == L.ERR_STATE
    assert e.lib.mfh_stress_field_load(e.h, L.FIELD_LOAD_STRESS, ptr(s), None, 0, ptr(out)) == L.ERR_STATE
    e.close()
    # MFH_ERR_UNSUPPORTED: a row-partitioned context; another operator than elasticity for the stress-field load
    V, T = _mesh(2)
    p = M.Context(0)
    p.mesh_set(2, 1, T, V, n_owned=len(V) - 3)
    p.material_isotropic(200.0, 0.3)
    po = np.empty((len(V), 2))
    ps = np.zeros((len(T), 3))
    assert p.lib.mfh_body_force_load(p.h, L.BODY_CONSTANT, ptr(b), None, 0, ptr(po)) == L.ERR_UNSUPPORTED
    assert p.lib.mfh_stress_field_load(p.h, L.FIELD_LOAD_STRESS, ptr(ps), None, 0, ptr(po)) == L.ERR_UNSUPPORTED
    p.close()
    q = M.Context(0)
    q.mesh_build(T, V, 2)
    q.set_operator(M.OP_LAPLACIAN)
    assert q.n_elem == c.n_elem and q.n_node == c.n_node
    assert q.lib.mfh_stress_field_load(q.h, L.FIELD_LOAD_STRESS, ptr(s), None, 0, ptr(out)) == L.ERR_UNSUPPORTED
    _close(q.body_force_load(f["b_node"], rho), r.body_force_load(f["b_node"], rho), "body force on a scalar-operator context")
    q.close()
    # the context works afterwards
    _close(c.body_force_load(f["b_elem"], rho), r.body_force_load(f["b_elem"], rho), "after the refusals")
    _close(c.stress_field_load(f["sigma"]), r.stress_field_load(f["sigma"]), "after the refusals")


# ------------------------------------------------------------------------------------------------ physics, through Simulator
def test_hanging_column():
    """P2, nu = 0, a 1 x 1 x L column clamped at z = 0 under a body force rho g e_z: u_z = rho g / E (L z - z^2 / 2), u_x = u_y = 0 -- a quadratic
    field, so the P2 solution is the analytic one"""
    from meshfem_amd import grid
    from meshfem_amd.linear_elasticity import Simulator
    L_, E, rho, g = 3.0, 50.0, 2.5, 9.81
    V, T = grid.grid_tet_mesh(2, 2, 4, [0, 0, 0], [1, 1, L_])
    sim = Simulator(T, V, 2)
    sim.setIsotropicMaterial(E, 0.0)
    sim.applyDirichletBox([-1e-9, -1e-9, -1e-9], [1 + 1e-9, 1 + 1e-9, 1e-9], [0, 0, 0])
    sim.rtol = 1e-12
    f = sim.gravityLoad([0, 0, g], rho)
    u = sim.solve(f)
    z = sim.nodes()[:, 2]
    ref = np.zeros_like(u)
    ref[:, 2] = rho * g / E * (L_ * z - 0.5 * z * z)
    _close(u, ref, "hanging column", 1e-9)
    assert np.array_equal(f, sim.bodyForceLoad(np.array([0, 0, g]), np.full(sim.numElements(), rho)))
    sim.ctx.close()


def _sim(dim, deg, E=70.0, nu=0.3):
    from meshfem_amd.linear_elasticity import Simulator
    V, T = _mesh(dim)
    sim = Simulator(T, V, deg)
    sim.setIsotropicMaterial(E, nu)
    sim.applyNoRigidMotionConstraint()
    sim.rtol = 1e-12
    return sim


@pytest.mark.parametrize("dim,deg", CASES)
def test_free_thermal_expansion(dim, deg):
    """uniform dT on a free body: u = alpha dT (x - mean of the nodes) -- the no-rigid-motion rows remove the nodal mean of u and of x cross u --
    and no stress"""
    E, alpha, dT = 70.0, 2.0e-3, 35.0
    sim = _sim(dim, deg, E)
    dTe = np.full(sim.numElements(), dT)
    u = sim.solve(sim.thermalLoad(alpha, dTe))
    x = sim.nodes()
    _close(u, alpha * dT * (x - x.mean(axis=0)), "%dD P%d free expansion" % (dim, deg), 1e-9)
    s = sim.thermalStress(u, alpha, dTe)
    assert s.shape == sim.stressField(u).shape
    print("thermal stress %.2e of E alpha dT" % (np.abs(s).max() / (E * alpha * dT)))
    assert np.abs(s).max() <= 1e-9 * E * alpha * dT
    sim.ctx.close()


@pytest.mark.parametrize("dim,deg", CASES)
def test_bimaterial_strip_is_self_equilibrated(dim, deg):
    """two expansion coefficients, one dT, no external load: the thermal stress does not vanish, its volume integral does, component by
    component (test the weak equilibrium with the linear fields v = x_j e_i, which lie in the space): up to the solver's residual"""
    E, dT = 70.0, 35.0
    sim = _sim(dim, deg, E)
    c = sim.ctx
    centroid = sim.nodes()[c.elem_nodes()[:, :dim + 1]].mean(axis=1)
    alpha = np.where(centroid[:, 0] < np.median(centroid[:, 0]), 1.0e-3, 3.0e-3)
    u = sim.solve(sim.thermalLoad(alpha, dT))
    s = sim.thermalStress(u, alpha, dT)
    scale = np.abs(s).max()
    assert scale >= 1e-2 * E * 2.0e-3 * dT
    integral = (c.elem_volumes()[:, None] * s.mean(axis=1)).sum(axis=0)
    print("%dD P%d: max|s| %.3e, integral %.2e of max|s| vol" % (dim, deg, scale, np.abs(integral).max() / (scale * c.elem_volumes().sum())))
    assert np.abs(integral).max() <= 1e-9 * scale * c.elem_volumes().sum()
    sim.ctx.close()


def test_centrifugal_load_and_transient_load():
    """the centrifugal field is linear in x: the NODE flavour integrates it exactly, so the load is that of the restatement fed the same nodal
    field, and its total is mass omega^2 (centroid - axis); transient(load=...) takes a volume load as it stands"""
    from meshfem_amd import grid
    from meshfem_amd.linear_elasticity import Simulator
    V, T = grid.grid_tet_mesh(2, 2, 2, [0, 0, 0], [1, 1, 1])
    sim = Simulator(T, V, 2)
    sim.setIsotropicMaterial(50.0, 0.3)
    omega, p0, axis, rho = 3.0, np.array([0.2, -0.1, 0.0]), np.array([0.0, 0.0, 2.0]), 1.5
    f = sim.centrifugalLoad(omega, p0, axis, rho)
    x = sim.nodes() - p0
    x[:, 2] = 0.0
    r = R.Mesh(3, 2, sim.elements(), sim.nodes())
    _close(f, r.body_force_load(omega ** 2 * x, np.full(len(T), rho)), "centrifugal load")
    total = rho * omega ** 2 * (np.array([0.5, 0.5, 0.5]) - p0) * np.array([1.0, 1.0, 0.0])
    assert np.abs(f.sum(axis=0) - total).max() <= 1e-12 * np.abs(total).max()
    sim.applyDirichletBox([-1e-9, -1e-9, -1e-9], [1 + 1e-9, 1 + 1e-9, 1e-9], [0, 0, 0])
    g = sim.gravityLoad([0, 0, -1.0], rho)
    res = sim.transient(0.1, 3, density=rho, load=g, rtol=1e-10)
    assert sim.transient_info["stepsDone"] == 3 and res["u"].shape == (sim.numNodes(), 3) and res["u"][:, 2].min() < 0
    sim.ctx.close()


# ------------------------------------------------------------------------------------------------ above the grid cap
@pytest.mark.timeout(120)
def test_grid_stride_path():
    """the launchers cap a grid at 2048 workgroups of 256 lanes = 524 288 DoF rows per sweep: grid_tet_mesh(40, 40, 40) at degree 2 (1 536 000 tets,
    2 214 641 nodes) runs the `+= gridDim.x * 256` branch four times and a fifth, partial stride. CONSTANT and NODE flavours against the restatement
    (vectorised numpy: most of this test's ten seconds)."""
    import meshfem_amd as M
    from meshfem_amd import grid
    V, T = grid.grid_tet_mesh(40, 40, 40, [0, 0, 0], [1, 1, 1])
    V = U.perturbed(V, 0.05 / 40)                       # (0.15 h inverts a few tets of the hex subdivision)
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    assert c.n_node > 2048 * 256 and c.n_node % (2048 * 256) != 0
    r = R.Mesh(3, 2, c.elem_nodes(), c.node_positions())
    rng = np.random.default_rng(90)
    b, rho, b_node = rng.standard_normal(3), rng.uniform(0.5, 2.0, c.n_elem), rng.standard_normal((c.n_node, 3))
    _close(c.body_force_load(b, rho), r.body_force_load(b, rho), "constant, above the cap")
    _close(c.body_force_load(b_node, rho), r.body_force_load(b_node, rho), "node, above the cap")
    c.close()
