"""The element-integral kernels launched through LoadArgs / MFH_DISPATCH (mfh_kernels.hip) against FP64 references, in every
instantiated flavour and past their grid caps: k_constant_strain_load (with and without deltaP), k_average_strain (strain, stress,
uFixed / deltaP, addStrain and the `integral` reduction behind mfh_integrated_stress), k_average_gradient, k_strain_field,
k_boundary_strain_field, k_apply_delta_K, k_mutual_energies (with and without deltaP), k_mutual_energy_differential, and the
Neumann load of the ABI.

References: tests/element_integrals_util.py (batched restatements, pinned to the oracle's literal functions by
tests/test_element_integrals_reference.py) on the flavour grid; the oracle's literal functions on the one- and two-element meshes;
closed forms in FP64 / longdouble above the grid caps.

Bounds, from the project: RTOL = 1e-12 of the largest reference entry for the undifferentiated quantities
(test_strain_and_stress_interpolant_fields_match_oracle), HIP_RTOL = 1e-11 for the delta kernels (test_shape_derivatives.py). For
the scalar reductions the bound is relative to the sum of the absolute per-element terms of the reference (the rounding of a sum in
any order scales with it, not with the possibly cancelling result). One load is zero by construction -- constantStrainLoad with one
tensor on a periodic mesh, where every DoF sums a closed star -- and is bounded relative to the largest entry of the same load
without the DoF map, i.e. the size of the terms that cancel.

mfh_neumann_load forms its vector on the host; k_neumann_load only runs inside a solve (the load stays on the device), so the Neumann
check here pins the ABI function and the boundary tables it shares with the kernel, not the kernel's atomics."""
import numpy as np
import pytest

import element_integrals_util as U
import meshfem_amd as M
from meshfem_amd import grid
from oracle import meshfem_oracle as O
from test_shape_derivatives import HIP_RTOL

pytestmark = pytest.mark.gpu
# time limits: the slowest small case took 0.3 s and the tests above the caps 4.9 s (2D) and 7.3 s (3D) on an MI355X box; 60 s and 120 s leave
# more than the usual factor 3 for a loaded machine and for a slower host under the numpy references

RTOL = 1e-12
CASES = [(3, 2), (3, 1), (2, 2), (2, 1)]
CAP = 8192 * 256            # launch_*: grid_for(nElem, 8192) blocks of 256 lanes, the largest cap of the family


def _close(got, ref, tol, what, scale=None):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = np.abs(ref).max() if scale is None else scale
    err = np.abs(got - ref).max()
    assert np.all(np.isfinite(got)) and np.all(scale > 0) and np.all(np.abs(got - ref) <= tol * scale), \
        "%s: err %.3e > %.0e x scale %.3e" % (what, err, tol, np.max(scale))


_MESHES = {}


def _mesh(dim, deg):
    """3D: 3 x 3 x 3 cells, 648 tets, 216 boundary triangles; 2D: 13 x 11 quads, 572 triangles, 48 boundary edges: three workgroups, the
    last one with a partial wave (the conditions asserted in the flavour test; larger meshes only add reference work). Interior vertices
    moved by up to 10 % of the cell edge, so that no two elements of a cell have the same shape and tensor record. Returns the oracle's
    FEMMesh (node numbering, boundary elements) and its periodic DoF map; cached per (dim, deg)."""
    if (dim, deg) not in _MESHES:
        V, T = grid.grid_tet_mesh(3, 3, 3) if dim == 3 else grid.grid_tri_mesh(13, 11)
        V = U.perturbed(V, 0.1)
        mesh = O.FEMMesh(T, V, deg)
        dof, n_dof, _ = O.periodic_dofs_for_nodes(mesh)
        _MESHES[dim, deg] = (V, np.asarray(T), mesh, dof, n_dof)
    return _MESHES[dim, deg]


def _general_strain(dim, rng):
    cs = rng.uniform(0.2, 1.0, O.flat_len(dim)) * rng.choice([-1.0, 1.0], O.flat_len(dim))
    assert np.all(cs != 0)                                                 # every shear entry takes part
    return cs


class Reference:
    """What every entry point must return, from the batched references: (value, scale or None = its largest entry)."""

    def __init__(self, s, mesh, traction, cancelling_load=False):
        self.s, self.mesh, self.traction, self.N = s, mesh, traction, s.N
        self.free = U.ElemSet(s.N, s.deg, s.en, mesh.verts, s.D) if cancelling_load else None

    def load(self, cs, dp=None):
        scale = None if self.free is None else np.abs(U.constant_strain_load(self.free, U.unflatten(self.N, cs), dp)).max()
        return U.constant_strain_load(self.s, U.unflatten(self.N, cs), dp), scale

    def neumann_load(self):
        m, s = self.mesh, self.s
        w = O.integrated_shape_functions(s.deg, s.K - 1)
        bvol, _ = m.bdry_elem_geometry()
        out = np.zeros((s.n_dof, s.N))
        np.add.at(out, s.dof[m.bdry_elem_nodes], (w[None, :] * bvol[:, None])[:, :, None] * self.traction[:, None, :])
        return out

    def apply_delta_K(self, u, dp):
        return U.apply_delta_K(self.s, u, dp)

    def average_strain(self, u, stress=False):
        e = U.average_strain(self.s, u)
        return self.s.stress(e) if stress else e

    def average_gradient(self, u0):
        return U.average_gradient(self.s, u0)

    def strain_field(self, u, stress):
        return U.strain_field(self.s, u, stress)

    def boundary_strain_field(self, u, stress):
        return U.boundary_strain_field(self.s, u, self.mesh.bdry_parent, self.mesh.bdry_elem_verts, stress)

    def delta_average_strain(self, u, du, dp, stress=False):
        e = U.delta_average_strain(self.s, u, du, dp)
        return self.s.stress(e) if stress else e

    def integrated_stress(self, u, cs):
        return U.longdouble_sum(U.integrated_stress_terms(self.s, u, cs))

    def mutual_energies(self, w, dp=None):
        return U.longdouble_sum(U.mutual_energy_terms(self.s, w, dp))

    def differential(self, w):
        return U.mutual_energy_differential(self.s, w, len(self.mesh.verts))


class LiteralReference(Reference):
    """The same from the oracle's literal functions (the scales of the reductions still come from the batched terms)."""

    def __init__(self, sim, traction):
        Reference.__init__(self, U.ElemSet.from_sim(sim), sim.mesh, traction)
        self.sim = sim
        sim.neumannTraction[:] = traction

    def load(self, cs, dp=None):
        cs = O.unflatten_sym(self.N, cs)
        return (self.sim.constantStrainLoad(cs) if dp is None else O.delta_constant_strain_load(self.sim, cs, dp)), None

    def neumann_load(self):
        return self.sim.neumannLoad()

    def apply_delta_K(self, u, dp):
        return O.apply_delta_stiffness_matrix(self.sim, u, dp)

    def average_strain(self, u, stress=False):
        return self.sim.averageStressField(u) if stress else self.sim.averageStrainField(u)

    def average_gradient(self, u0):
        return O.grad_u_average(self.mesh, u0)

    def strain_field(self, u, stress):
        return self.sim.strainField(u, stress=stress)

    def boundary_strain_field(self, u, stress):
        return O.boundary_strain_field(self.sim, u, stress=stress)

    def delta_average_strain(self, u, du, dp, stress=False):
        e = O.delta_average_strain_field(self.sim, u, du, dp)
        return np.stack([self.sim.elem_D(k).double_contract_flat(e[k]) for k in range(len(e))]) if stress else e

    def integrated_stress(self, u, cs):
        eps = self.sim.averageStrainField(u)
        add = 0.0 if cs is None else np.asarray(cs)
        val = sum(self.sim.vol[e] * self.sim.elem_D(e).double_contract_flat(eps[e] + add) for e in range(len(eps)))
        return val, Reference.integrated_stress(self, u, cs)[1]

    def mutual_energies(self, w, dp=None):
        return O.mutual_energies(self.sim, w, dp), Reference.mutual_energies(self, w, dp)[1]

    def differential(self, w):
        return np.transpose(O.homogenized_elasticity_tensor_discrete_differential(self.sim, w, base_cell_volume=1.0), (2, 3, 0, 1))


def _context(mesh, deg, setter, dof=None, n_dof=None, options=()):
    c = M.Context(0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(mesh.elems, mesh.verts, deg)
    setter(c)
    if dof is not None:
        assert c.apply_periodic_conditions() == n_dof and np.array_equal(c.get_dof_map()[0], dof)
    # the numbering the references are written in: nodes, boundary elements and their parents
    assert np.array_equal(c.elem_nodes(), mesh.elem_nodes) and np.array_equal(c.boundary_elem_nodes(), mesh.bdry_elem_nodes)
    assert np.array_equal(c.boundary_elem_parents(), mesh.bdry_parent)
    return c


def _face_traction(mesh, rng):
    """a different traction on every boundary element of the face x = max, zero elsewhere: [nBE, N]"""
    x = mesh.verts[mesh.bdry_elem_verts][:, :, 0]
    on = np.flatnonzero((x > mesh.verts[:, 0].max() - 1e-9).all(axis=1))
    assert len(on) > 0
    t = np.zeros((len(mesh.bdry_elem_verts), mesh.N))
    t[on] = rng.normal(size=(len(on), mesh.N))
    return on, t


def check_every_entry_point(c, ref, rng, on, label, repeat=True):
    """Every Context method of the family on independent random inputs. Loads are per DoF (n_dof rows), fields per node / element / vertex."""
    dim, fl = c.dim, O.flat_len(c.dim)
    nn, nvert = c.n_node, c.n_vert
    u, du = rng.normal(size=(nn, dim)), rng.normal(size=(nn, dim))
    w = [rng.normal(size=(nn, dim)) * 0.1 for _ in range(fl)]
    dp = rng.normal(size=(nvert, dim)) * 0.05                              # the boundary moves too
    cs = _general_strain(dim, rng)
    tag = lambda what: "%s: %s" % (label, what)

    # ---- loads, per DoF
    want, scale = ref.load(cs)
    got = c.constant_strain_load(cs)                                       # fresh context: k_constant_strain_load
    assert got.shape == (c.n_dof, dim)
    _close(got, want, RTOL, tag("constant_strain_load"), scale)
    want, scale = ref.load(cs, dp)
    got = c.delta_constant_strain_load(cs, dp)
    _close(got, want, HIP_RTOL, tag("delta_constant_strain_load"), scale)
    if repeat:
        _close(c.delta_constant_strain_load(cs, dp), got, HIP_RTOL, tag("delta_constant_strain_load twice"), np.abs(want).max() if scale is None else scale)
    c.bc_neumann_elements(on, ref.traction[on])
    _close(c.neumann_load(), ref.neumann_load(), RTOL, tag("neumann_load"))
    want = ref.apply_delta_K(u, dp)
    got = c.apply_delta_K(u, dp)
    assert got.shape == (c.n_dof, dim)
    _close(got, want, HIP_RTOL, tag("apply_delta_K"))
    if repeat:
        _close(c.apply_delta_K(u, dp), got, HIP_RTOL, tag("apply_delta_K twice"), np.abs(want).max())

    # ---- per-element fields: the DoF map must not reach them
    _close(c.average_strain(u), ref.average_strain(u), RTOL, tag("average_strain"))
    _close(c.average_stress(u), ref.average_strain(u, stress=True), RTOL, tag("average_stress"))
    _close(c.average_gradient(u[:, 0]), ref.average_gradient(u[:, 0]), RTOL, tag("average_gradient"))
    for stress in (False, True):
        _close(c.strain_field(u, stress), ref.strain_field(u, stress), RTOL, tag("strain_field stress=%d" % stress))
        _close(c.boundary_strain_field(u, stress), ref.boundary_strain_field(u, stress), RTOL, tag("boundary_strain_field stress=%d" % stress))
        _close(c.delta_average_strain(u, du, dp, stress), ref.delta_average_strain(u, du, dp, stress), HIP_RTOL,
               tag("delta_average_strain stress=%d" % stress))

    # ---- reductions: bounds relative to the sum of the absolute terms
    for add in (None, cs):
        want, scale = ref.integrated_stress(u, add)
        got = c.integrated_stress(u, add)
        _close(got, want, RTOL, tag("integrated_stress cstrain=%d" % (add is not None)), scale)
        if repeat:
            _close(c.integrated_stress(u, add), got, RTOL, tag("integrated_stress twice"), scale)
    for d, tol in ((None, RTOL), (dp, HIP_RTOL)):
        want, scale = ref.mutual_energies(w, d)                             # both triangles, each from its own terms
        got = c.mutual_energies(w, d)
        assert got.shape == (fl, fl) and np.array_equal(got, got.T)
        _close(got, want, tol, tag("mutual_energies deltaP=%d" % (d is not None)), scale)
        if repeat:
            _close(c.mutual_energies(w, d), got, tol, tag("mutual_energies twice"), scale)

    # ---- the one-form, per vertex: [pairs] = the upper triangle ij <= kl, row-major
    want = ref.differential(w)                                             # [fl, fl, nVert, N]
    one = c.mutual_energy_differential(w)
    iu = np.triu_indices(fl)
    assert one.shape == (len(iu[0]), nvert, dim)
    _close(one, want[iu], HIP_RTOL, tag("mutual_energy_differential"))
    _close(one, np.transpose(want, (1, 0, 2, 3))[iu], HIP_RTOL, tag("mutual_energy_differential, lower triangle"))
    if repeat:
        _close(c.mutual_energy_differential(w), one, HIP_RTOL, tag("mutual_energy_differential twice"), np.abs(want).max())
    dM, scale = ref.mutual_energies(w, dp)
    _close(np.einsum("pvc,vc->p", one, dp), dM[iu], HIP_RTOL, tag("one-form . deltaP"), np.abs(want).max() * np.abs(dp).sum())

    # ---- the constant-strain load once the matrix-free operator's lists exist: the element routine of the cluster operator
    info = c.matrix_free_info()
    if info["active"] and info["mode"] == 4:
        want, scale = ref.load(cs)
        _close(c.constant_strain_load(cs), want, RTOL, tag("constant_strain_load, cluster lists"), scale)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("dim,deg", CASES)
def test_every_flavour_on_several_blocks(dim, deg, mode, periodic):
    """All 12 instantiations of every kernel of the family, fed by the six material modes of k_geometry, on a mesh of several workgroups
    with a partial last wave (asserted below), with and without the periodic DoF map."""
    V, T, mesh, dof, n_dof = _mesh(dim, deg)
    setter, D = U.material(mode, dim, len(T))
    c = _context(mesh, deg, setter, dof if periodic else None, n_dof)
    assert c.n_elem > 512 and c.n_elem % 256 != 0 and c.n_elem % 64 != 0 and c.n_bdry_elem % 64 != 0
    assert (c.n_dof < c.n_node) == periodic
    s = U.ElemSet(dim, deg, mesh.elem_nodes, V, D, dof if periodic else None, n_dof if periodic else None)
    assert s.vol.min() > 0 and s.vol.max() > 1.5 * s.vol.min()             # the elements differ
    rng = np.random.default_rng(1000 * dim + 100 * deg + 10 * U.MODES.index(mode) + periodic)
    on, t = _face_traction(mesh, rng)
    ref = Reference(s, mesh, t, cancelling_load=periodic and mode in ("iso", "general", "ortho"))
    check_every_entry_point(c, ref, rng, on, "%dD P%d %s periodic=%d" % (dim, deg, mode, periodic))
    c.close()


@pytest.mark.timeout(60)
@pytest.mark.parametrize("dim,deg", CASES)
def test_option_deterministic_keeps_the_results(dim, deg):
    """Option deterministic 1 orders the sums of the assembly, the operator and the PCG (docs/design/04_2, 04_4a, 04_5); the kernels of this
    family keep their atomics in arrival order (docs/design/04_9_shape_derivatives.md), so the option must leave their results where they
    were -- to the same bounds, not bit for bit -- and it sends the constant-strain load to k_constant_strain_load even when the cluster lists exist."""
    V, T, mesh, dof, n_dof = _mesh(dim, deg)
    setter, D = U.material("ortho_field", dim, len(T))
    c = _context(mesh, deg, setter, options=(("deterministic", 1),))
    c.matrix_free_info()
    rng = np.random.default_rng(77 + dim + deg)
    on, t = _face_traction(mesh, rng)
    check_every_entry_point(c, Reference(U.ElemSet(dim, deg, mesh.elem_nodes, V, D), mesh, t), rng, on, "%dD P%d deterministic" % (dim, deg))
    c.close()


@pytest.mark.timeout(60)
@pytest.mark.parametrize("dim,deg", CASES)
def test_one_and_two_element_meshes_match_the_literal_oracle(dim, deg):
    """Grids smaller than one wave: every quantity against the oracle's literal functions, per-element general tensors."""
    for n in (1, 2):
        V, T = grid.grid_tet_mesh(1, 1, 1) if dim == 3 else grid.grid_tri_mesh(1, 1)
        rng = np.random.default_rng(10 * dim + deg + n)
        T = np.asarray(T)[:n]
        used = np.unique(T)
        remap = np.full(len(V), -1)
        remap[used] = np.arange(len(used))
        V, T = V[used] + 0.05 * rng.normal(size=(len(used), dim)), remap[T]
        sim = O.Simulator(T, V, deg)
        Ds = np.stack([U.spd(rng, O.flat_len(dim)) for _ in range(n)])
        sim.set_material_field([O.ElasticityTensor(dim, d) for d in Ds])
        c = _context(sim.mesh, deg, lambda ctx: ctx.material_tensor_field(Ds))
        assert c.n_elem == n
        t = rng.normal(size=(len(sim.mesh.bdry_elem_verts), dim))          # a traction on every boundary element
        check_every_entry_point(c, LiteralReference(sim, t), rng, np.arange(len(t)), "%dD P%d, %d element(s)" % (dim, deg, n))
        c.close()


# ------------------------------------------------------------------------------------------------ past the grid caps
def _volumes(V, T):
    """signed volumes from the vertex coordinates (determinant formula), on the host"""
    E = V[T[:, 1:]] - V[T[:, :1]]
    return np.linalg.det(E) / (6.0 if V.shape[1] == 3 else 2.0)


def _windows(n_elem):
    """4 096 elements at the start, around the first element of the second grid stride, and at the end"""
    return [np.arange(0, 4096), np.arange(CAP - 2048, CAP + 2048), np.arange(n_elem - 4096, n_elem)]


def check_above_the_cap(c, V, T, D, rng, label):
    """Closed forms for affine fields, the dilation / translation identities and random inputs on windows; D: [nElem, fl, fl]."""
    dim, fl, deg = c.dim, O.flat_len(c.dim), c.deg
    n_elem, nn = c.n_elem, c.n_node
    assert n_elem == len(T) > CAP + 256 and n_elem % 256 != 0             # every kernel strides; the last stride is partial
    tag = lambda what: "%s: %s" % (label, what)
    dbl = np.where(np.arange(fl) < dim, 1.0, 2.0)
    vol = _volumes(V, T)
    assert vol.min() > 0
    pos = c.node_positions()
    en = c.elem_nodes().astype(np.int64)
    assert np.array_equal(en[:, :dim + 1], T) and np.array_equal(pos[:len(V)], V)

    # ---- affine fields u = A x + b: strains sym(A) everywhere, exactly representable (P2 edge nodes are midpoints)
    A, b = rng.normal(size=(dim, dim)), 0.1 * rng.normal(size=dim)
    u = pos @ A.T + b
    eA = U.flatten(dim, 0.5 * (A + A.T))
    sig = np.einsum("erc,c->er", D, eA * dbl)                              # C_e : sym(A)
    _close(c.average_strain(u), np.broadcast_to(eA, (n_elem, fl)), HIP_RTOL, tag("affine average_strain"))
    _close(c.average_stress(u), sig, HIP_RTOL, tag("affine average_stress"))
    sf = c.strain_field(u)
    _close(sf, np.broadcast_to(eA, sf.shape), HIP_RTOL, tag("affine strain_field"))
    sf = c.strain_field(u, True)
    _close(sf, np.broadcast_to(sig[:, None, :], sf.shape), HIP_RTOL, tag("affine stress field"))
    bf = c.boundary_strain_field(u)
    _close(bf, np.broadcast_to(eA, bf.shape), HIP_RTOL, tag("affine boundary_strain_field"))
    _close(c.average_gradient(u[:, 0].copy()), np.broadcast_to(A[0], (n_elem, dim)), HIP_RTOL, tag("affine average_gradient"))
    del sf, bf
    cs = _general_strain(dim, rng)
    for add in (None, cs):
        terms = vol[:, None] * (sig if add is None else np.einsum("erc,c->er", D, (eA + add) * dbl))
        want, scale = U.longdouble_sum(terms)
        _close(c.integrated_stress(u, add), want, HIP_RTOL, tag("affine integrated_stress cstrain=%d" % (add is not None)), scale)
    As = rng.normal(size=(fl, dim, dim)) * 0.3
    w = [pos @ As[k].T for k in range(fl)]
    Gd = np.stack([U.flatten(dim, O.canonical_strain(dim, k) + 0.5 * (As[k] + As[k].T)) for k in range(fl)]) * dbl
    terms = vol[:, None, None] * np.einsum("ic,ecj->eij", Gd, np.einsum("ecd,jd->ecj", D, Gd))
    want, scale = U.longdouble_sum(terms)
    Mw = c.mutual_energies(w)
    _close(Mw, want, HIP_RTOL, tag("affine mutual_energies"), scale)
    del terms

    # ---- dilation delta_p = x (every length scales) and translations, as at 16^3 in test_shape_derivatives.py
    ur = rng.normal(size=(nn, dim))
    Ku = c.apply_K(ur.ravel()).reshape(nn, dim)
    _close(c.apply_delta_K(ur, V), (dim - 2) * Ku, HIP_RTOL, tag("dilation (delta K) u = (dim - 2) K u"), np.abs(Ku).max())
    shift = np.tile(rng.normal(size=dim), (len(V), 1))
    assert np.abs(c.apply_delta_K(ur, shift)).max() < 1e-10 * np.abs(Ku).max(), tag("translation (delta K) u")
    load = c.constant_strain_load(cs)
    _close(c.delta_constant_strain_load(cs, V), (dim - 1) * load, HIP_RTOL, tag("dilation of the constant-strain load"), np.abs(load).max())
    e = c.average_strain(ur)
    _close(c.delta_average_strain(ur, np.zeros_like(ur), V), -e, HIP_RTOL, tag("dilation of the strain"), np.abs(e).max())
    wr = [rng.normal(size=(nn, dim)) * 0.05 for _ in range(fl)]
    one = c.mutual_energy_differential(wr)
    assert np.abs(one.sum(axis=1)).max() < 1e-9 * np.abs(one).max() * len(V) ** 0.5, tag("one-form sums to zero")
    dp = rng.normal(size=V.shape) * 0.01
    dM = c.mutual_energies(wr, dp)
    iu = np.triu_indices(fl)
    _close(np.einsum("pvc,vc->p", one, dp), dM[iu], HIP_RTOL, tag("one-form . deltaP"), np.abs(dM).max())
    del one
    zero = [np.zeros((nn, dim))] * fl
    M0 = c.mutual_energies(zero)
    _close(c.mutual_energies(zero, V), dim * M0, HIP_RTOL, tag("dilation of the volume term"), np.abs(M0).max())

    # ---- random inputs on three windows of elements against the batched reference of just those elements
    du = rng.normal(size=(nn, dim))
    got_e, got_f, got_d = c.average_strain(ur), c.strain_field(ur, True), c.delta_average_strain(ur, du, dp, True)
    got_K, got_l, got_dl = c.apply_delta_K(ur, dp), load, c.delta_constant_strain_load(cs, dp)
    star = np.bincount(en.ravel(), minlength=nn)
    for k, win in enumerate(_windows(n_elem)):
        s = U.ElemSet(dim, deg, en[win], V, D[win], n_dof=nn)
        _close(got_e[win], U.average_strain(s, ur), HIP_RTOL, tag("window %d average_strain" % k))
        _close(got_f[win], U.strain_field(s, ur, True), HIP_RTOL, tag("window %d stress field" % k))
        _close(got_d[win], s.stress(U.delta_average_strain(s, ur, du, dp)), HIP_RTOL, tag("window %d delta_average_stress" % k))
        # scatter outputs on the DoFs whose whole element star lies inside the window
        whole = np.flatnonzero((np.bincount(en[win].ravel(), minlength=nn) == star) & (star > 0))
        assert len(whole) > 100
        _close(got_K[whole], U.apply_delta_K(s, ur, dp)[whole], HIP_RTOL, tag("window %d apply_delta_K" % k))
        _close(got_l[whole], U.constant_strain_load(s, U.unflatten(dim, cs))[whole], HIP_RTOL, tag("window %d constant_strain_load" % k))
        _close(got_dl[whole], U.constant_strain_load(s, U.unflatten(dim, cs), dp)[whole], HIP_RTOL, tag("window %d delta_constant_strain_load" % k))


@pytest.mark.timeout(120)
def test_above_the_grid_caps_2d():
    """launch_* in mfh_kernels.hip cap the grid at 1024 x 256 elements for the integral reduction of k_average_strain, 4096 x 256 for
    k_mutual_energies / k_mutual_energy_differential and 8192 x 256 = 2 097 152 for the rest (k_constant_strain_load: 8192 x 256
    (element, node) pairs): above that every kernel runs its `+= gridDim.x * 256` branch. 725 x 724 quads -> 2 099 600 triangles, P1 and
    P2, per-element general tensors. Closed forms stay inside the bound at this size: for 2.1 M terms the float64 and the longdouble
    sum of the reference differ by 3e-14 of the sum of the absolute terms (checked on the host).
    The cell is centred at the origin and the offset b of the affine fields is small: sum_i u_i grad phi_i cancels terms of size
    max|u| max|grad phi| ~ |A| L / h down to |A|, so any FP64 evaluation of an affine strain is off by a multiple of eps L / h whatever the
    kernel does. With L / h = 725 the host's own FP64 evaluation (element_integrals_util.strain_field, P2) misses sym(A) by up to
    9.6e-12 of its largest entry on the cell [0, 1]^2 with |b| ~ 1, and by 2.2e-12 on this one: the affine bound 1e-11 then tests the kernel."""
    V, T = grid.grid_tri_mesh(725, 724, [-0.5, -0.5], [0.5, 0.5])
    V = U.perturbed(V, 0.15 / 725)
    T = np.ascontiguousarray(T, dtype=np.int64)
    rng = np.random.default_rng(21)
    A = rng.normal(size=(len(T), 3, 3))
    D = A @ np.transpose(A, (0, 2, 1)) + 3.0 * np.eye(3)
    del A
    for deg in (1, 2):
        c = M.Context(0)
        c.mesh_build(T, V, deg)
        c.material_tensor_field(D)
        check_above_the_cap(c, V, T, D, rng, "2D P%d" % deg)
        c.close()


@pytest.mark.timeout(120)
def test_above_the_grid_caps_3d():
    """45 x 45 x 44 cells -> 2 138 400 P2 tets (above 8192 x 256 + 256, not a multiple of 256), per-element orthotropic field: the strided
    regime configs[2..4] run every kernel of the family in."""
    V, T = grid.grid_tet_mesh(45, 45, 44, [0, 0, 0], [1.0, 1.0, 44.0 / 45.0])
    V = U.perturbed(V, 0.1 / 45)
    T = np.ascontiguousarray(T, dtype=np.int64)
    P = grid.synthetic_orthotropic_field(len(T), 3, seed=3)
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    c.material_ortho_field(P)
    check_above_the_cap(c, V, T, U.orthotropic_D(3, P), np.random.default_rng(22), "3D P2")
    c.close()
