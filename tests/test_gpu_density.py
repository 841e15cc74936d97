"""The per-element density on the device (mfh_set_density, mfh_mass_apply, mfh_mass_properties and the mass matrix of mfh_modes / mfh_newmark;
docs/design/04_15_density.md) against the numpy restatement tests/density_util.py, which tests/test_density_reference.py pins on the CPU.
Meshes: modes_util.SMALL (the 4 x 3 triangle grid and the 3 x 2 x 2 tet grid, P1 and P2, perturbed), the mid mesh once, one linear mesh past
the grid cap of the mass-property kernels. Fields: bimaterial (1 | 8 across the middle of x) and a seeded random one in [0.5, 4].
Bars:
  products, mass properties   1e-12 of scale: the standing bound of the project for applications (tests/test_gpu_volume_loads.py)
  modes                       those of tests/test_gpu_modes.py with M_rho in place of M: |lambda~ - lambda| <= sqrt(cond2(M_rho,ff)) rtol lambda,
                              host residuals <= 2 rtol, orthonormality <= max(10 x eigh's own defect, n eps)
  dynamics                    those of tests/test_gpu_dynamics.py: states <= 1e3 rtol, energies <= 1e2 rtol
Every solve is made once (functools.lru_cache) and shared by the tests that look at it."""
import ctypes as C
import functools

import numpy as np
import pytest

import meshfem_amd as M
from meshfem_amd import _lib as L
from meshfem_amd._lib import ptr

import density_util as DU
import dynamics_util as D
import modes_util as U

pytestmark = pytest.mark.gpu

TOL = 1e-12
RTOL = 1e-6                  # mode solves
DYN_RTOL = 1e-12             # Newmark's PCG
EPS = U.EPS
PRECONDS = {"jacobi": M.PRECOND_BLOCK_JACOBI, "two-level": M.PRECOND_TWO_LEVEL, "multigrid": M.PRECOND_MULTIGRID}
MASS_GRID_CAP = 512          # workgroups of k_mass_moments (mfh_internal.hh): one stride of the capped grid covers 512 x 256 elements


def _name(key):
    return key if isinstance(key, str) else "%dD-P%d" % key


def _is3d(key):
    return key == U.MID or key[0] == 3


def _context(key, precond="jacobi", options=(), field=None):
    V, T, deg, _ = U.mesh_arrays(key)
    c = M.Context(0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    c.set_preconditioner(PRECONDS[precond])
    if field is not None:
        c.set_density(DU.field(key, field))
    return c


def _rand(n, seed=5):
    return np.random.default_rng(seed).standard_normal(n)


def _scale_err(got, ref):
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / np.abs(ref).max())


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
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = self.alloc(a.nbytes)
        self.c.dev_memcpy(p, ptr(a), a.nbytes, 0)
        return p

    def down(self, p, shape):
        out = np.empty(shape)
        self.c.dev_memcpy(ptr(out), p, out.nbytes, 1)
        return out

    def free(self):
        for p in self.ptrs:
            self.c._ck(self.c.lib.mfh_debug_arena_free(self.c.h, C.c_void_p(p)))


# ------------------------------------------------------------------------------------------------ 1, 2: the product
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_mass_apply_against_the_restatement(key):
    c = _context(key)
    assert np.array_equal(c.node_positions(), U.fem_mesh(key).node_pos)          # the oracle's node numbering is the library's own
    assert np.array_equal(c.elem_nodes(), DU.mesh_tables(key)[0])
    x = _rand(c.dim * c.n_dof)
    for name in [None] + DU.FIELDS + [None]:                                    # unit density before any field and after clearing one
        c.set_density(None if name is None else DU.field(key, name))
        ref = DU.M_rho(key, name) @ x
        got = c.mass_apply(x)
        err = _scale_err(got, ref)
        print("%s %s: %.3e of scale" % (_name(key), name, err))
        assert err <= TOL
    # device pointers
    d = _Dev(c)
    try:
        c.set_density(None)
        rho = DU.field(key, "random")
        c._ck(c.lib.mfh_set_density(c.h, d.up(rho), len(rho), L.LOAD_ON_DEVICE))
        y = d.alloc(8 * x.size)
        c._ck(c.lib.mfh_mass_apply(c.h, d.up(x), y, L.LOAD_ON_DEVICE))
        got = d.down(y, x.shape)
        assert _scale_err(got, DU.M_rho(key, "random") @ x) <= TOL
        assert _scale_err(got, c.mass_apply(x)) <= 1e-14                        # (a quadratic context reassembles per call: the LDS adds are not ordered)
    finally:
        d.free()
    c.close()


def test_mass_apply_under_a_periodic_dof_map():
    """the unit cell with its interior perturbed, quadratic triangles: y = P^T M_rho P x"""
    import element_integrals_util as EU
    from meshfem_amd import grid
    V, T = grid.grid_tri_mesh(4, 3, [0, 0], [1, 1])
    V = EU.perturbed(V, 0.05)
    c = M.Context(0)
    c.mesh_build(T, V, 2)
    c.material_isotropic(U.E_MOD, U.NU)
    n_dof = c.apply_periodic_conditions()
    assert n_dof < c.n_node and c.n_dof == n_dof
    dof, _ = c.get_dof_map()
    en, pos = c.elem_nodes(), c.node_positions()
    rho = DU.density_field("bimaterial", en, pos, 2)
    assert rho.min() == 1.0 and rho.max() == 8.0
    c.set_density(rho)
    x = _rand(2 * n_dof)
    ref = DU.mass_matrix(2, 2, en, pos, rho, dof, n_dof) @ x
    err = _scale_err(c.mass_apply(x), ref)
    print("periodic 2D-P2: %.3e of scale" % err)
    assert err <= TOL
    c.close()


@pytest.mark.parametrize("name", DU.FIELDS)
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_mass_apply_is_the_body_force_load_of_a_nodal_field(key, name):
    """an identity on an older entry point: M_rho b = body_force_load(b_nodal, density=rho)"""
    c = _context(key, field=name)
    b = _rand((c.n_node, c.dim), 9)
    load = c.body_force_load(b, density=DU.field(key, name))
    err = _scale_err(c.mass_apply(b), load)
    print("%s %s: %.3e of scale" % (_name(key), name, err))
    assert err <= TOL
    c.close()


# ------------------------------------------------------------------------------------------------ 3: constant field = scalar
def _modes_and_end_state(key, rho, density):
    c = _context(key)
    c.fix_variables(U.clamp_vars(key))
    if rho is not None:
        c.set_density(rho)
    lam, _, _ = c.modes(4, density=density, rtol=1e-9, maxit=5000)
    i = D.case_inputs(key, "damped", 20)
    r = c.newmark(i["dt"], 20, u0=i["u0"], v0=i["v0"], f=i["f"], amplitude=i["amplitude"], density=density, damping=i["damping"], rtol=DYN_RTOL,
                  maxit=20000)
    c.close()
    return lam, np.concatenate([r["u"], r["v"], r["a"]])


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_constant_field_equals_the_scalar(key):
    n_elem = len(DU.mesh_tables(key)[0])
    lam_s, st_s = _modes_and_end_state(key, None, 1.7)
    lam_f, st_f = _modes_and_end_state(key, np.full(n_elem, 1.7), 1.0)
    e1, e2 = np.abs(lam_f / lam_s - 1).max(), np.linalg.norm(st_f - st_s) / np.linalg.norm(st_s)
    rho = DU.field(key, "random")
    lam_a, st_a = _modes_and_end_state(key, rho, 2.0)
    lam_b, st_b = _modes_and_end_state(key, 2.0 * rho, 1.0)
    e3, e4 = np.abs(lam_b / lam_a - 1).max(), np.linalg.norm(st_b - st_a) / np.linalg.norm(st_a)
    print("%s: field 1.7 vs scalar 1.7: lambda %.3e, state %.3e; scalar 2 vs doubled field: lambda %.3e, state %.3e" % (_name(key), e1, e2, e3, e4))
    assert max(e1, e2, e3, e4) <= 1e-10


# ------------------------------------------------------------------------------------------------ 4: modes of the bimaterial body
@functools.lru_cache(maxsize=None)
def _clamped(key, precond, nev):
    c = _context(key, precond, field="bimaterial")
    c.fix_variables(U.clamp_vars(key))
    out = c.modes(nev, rtol=RTOL, maxit=3000)
    c.close()
    return out


@functools.lru_cache(maxsize=None)
def _free(key, precond, nev):
    c = _context(key, precond, field="bimaterial")
    out = c.modes(nev, free=True, rtol=RTOL, maxit=3000)
    c.close()
    return out


MODE_CASES = [(k, "jacobi") for k in U.SMALL] + [(k, p) for k in U.SMALL if _is3d(k) for p in ("two-level", "multigrid")]


def _check_clamped(key, precond, nev):
    lam, X, info = _clamped(key, precond, nev)
    ref, _, cond, defect_ref = DU.clamped_truth(key, "bimaterial")
    bar = np.sqrt(cond) * RTOL * ref[:nev]
    err = np.abs(lam - ref[:nev])
    K, Mr = U.pencil(key)[0], DU.M_rho(key, "bimaterial")
    f = U.free_vars(key, U.clamp_vars(key))
    res = U.host_residuals(K[f][:, f], Mr[f][:, f], lam, X[:, f])
    defect = np.abs(X @ (Mr @ X.T) - np.eye(nev)).max()
    print("%s %s nev %d: %d iterations, max err / bar %.3e, host residuals %.3e (reported %.3e), defect %.3e (eigh's %.3e), note '%s'" %
          (_name(key), precond, nev, info["iterations"], (err / bar).max(), res.max(), info["maxResidual"], defect, defect_ref, info["note"]))
    assert info["converged"] == 1 and info["maxResidual"] <= RTOL
    assert np.all(np.diff(lam) >= 0)
    assert np.all(err <= bar)
    assert np.all(res <= 2 * RTOL)
    assert np.all(info["residuals"] <= 2 * res) and np.all(res <= 2 * info["residuals"])
    assert defect <= max(10 * defect_ref, X.shape[1] * EPS)
    assert np.all(X[:, U.clamp_vars(key)] == 0.0)


@pytest.mark.parametrize("nev", [1, 4, 7])
@pytest.mark.parametrize("key,precond", MODE_CASES, ids=_name)
def test_bimaterial_modes_clamped(key, precond, nev):
    _check_clamped(key, precond, nev)


def test_bimaterial_modes_mid_mesh():
    _check_clamped(U.MID, "multigrid", 4)
    assert _clamped(U.MID, "multigrid", 4)[2]["precondUsed"] == M.PRECOND_MULTIGRID


@pytest.mark.parametrize("nev", [1, 4, 7])
@pytest.mark.parametrize("key,precond", MODE_CASES, ids=_name)
def test_bimaterial_modes_free(key, precond, nev):
    lam, X, info = _free(key, precond, nev)
    K, Mr = U.pencil(key)[0], DU.M_rho(key, "bimaterial")
    pos = DU.mesh_tables(key)[1]
    nz = 6 if pos.shape[1] == 3 else 3
    ref, _, cond, defect_ref = DU.free_truth(key, "bimaterial")
    ref = ref[nz:nz + nev]
    bar = np.sqrt(cond) * RTOL * ref
    err = np.abs(lam - ref)
    res = U.host_residuals(K, Mr, lam, X)
    tol = max(10 * defect_ref, X.shape[1] * EPS)
    defect = np.abs(X @ (Mr @ X.T) - np.eye(nev)).max()
    Z = U.m_orthonormalise(U.rigid_modes(pos), Mr)
    rigid = np.abs(Z.T @ (Mr @ X.T)).max()
    print("%s %s nev %d: %d iterations, max err / bar %.3e, host residuals %.3e, defect %.3e, against the rigid modes %.3e (bar %.3e), note '%s'" %
          (_name(key), precond, nev, info["iterations"], (err / bar).max(), res.max(), defect, rigid, tol, info["note"]))
    assert info["converged"] == 1 and info["maxResidual"] <= RTOL
    assert np.all(err <= bar)
    assert np.all(res <= 2 * RTOL)
    assert defect <= tol
    assert rigid <= tol


# ------------------------------------------------------------------------------------------------ 5: Newmark with the bimaterial field
@functools.lru_cache(maxsize=None)
def _newmark_reference(key, case):
    K, Mr = U.pencil(key)[0], DU.M_rho(key, "bimaterial")
    i = D.case_inputs(key, case)
    return D.newmark_direct(K, Mr, D.free_of(key), i["dt"], i["n_steps"], i["u0"], i["v0"], i["f"], i["amplitude"], i["density"], i["damping"])


@pytest.mark.parametrize("case", ["undamped", "damped"])
@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_newmark_with_the_bimaterial_field(key, case):
    """100 steps of dynamics_util.case_inputs (scalar density 1.7 on top of the field) against the direct recurrence on (K, M_rho)"""
    i = D.case_inputs(key, case)
    c = _context(key, "multigrid" if _is3d(key) else "jacobi", field="bimaterial")
    c.fix_variables(U.clamp_vars(key))
    common = dict(u0=i["u0"], v0=i["v0"], density=i["density"], rtol=DYN_RTOL, maxit=20000, energies=True)
    r = c.newmark(i["dt"], i["n_steps"], f=i["f"], amplitude=i["amplitude"], damping=i["damping"], snapshot_stride=1, **common)
    free_run = c.newmark(i["dt"], i["n_steps"], **common)["energies"] if case == "undamped" else None
    c.close()
    Uref, Vref, Aref, Eref = _newmark_reference(key, case)
    err = D.rel_l2_rows(r["snapshots"], Uref)
    verr = D.rel_l2_rows(r["v"][None, :], Vref[-1:])
    eerr = (np.abs(r["energies"] - Eref).max(axis=0) / np.abs(Eref).max(axis=0)).max()
    Mr = DU.M_rho(key, "bimaterial")
    kin = 0.5 * i["density"] * (r["v"] @ (Mr @ r["v"]))
    kerr = abs(r["energies"][-1, 0] - kin) / np.abs(Eref[:, 0]).max()
    print("%s %s: snapshots %.3e, v %.3e (bar %.1e), energies %.3e, kinetic against 1/2 v.M_rho v %.3e (bar %.1e)" %
          (_name(key), case, err, verr, 1e3 * DYN_RTOL, eerr, kerr, 1e2 * DYN_RTOL))
    assert r["info"]["stepsDone"] == i["n_steps"]
    assert err <= 1e3 * DYN_RTOL and verr <= 1e3 * DYN_RTOL
    assert eerr <= 1e2 * DYN_RTOL
    assert kerr <= 1e2 * DYN_RTOL
    if free_run is not None:
        tot = free_run[:, 0] + free_run[:, 1]
        drift = np.abs(tot / tot[0] - 1).max()
        print("%s: energy drift of the unloaded run %.3e (bar %.1e)" % (_name(key), drift, 1e2 * DYN_RTOL))
        assert drift <= 1e2 * DYN_RTOL


# ------------------------------------------------------------------------------------------------ 6: mass properties
def _props_err(got, ref):
    return max(abs(got["mass"] / ref["mass"] - 1), np.abs(got["com"] - ref["com"]).max() / np.abs(ref["com"]).max(),
               _scale_err(got["second_moment"], ref["second_moment"]), _scale_err(got["inertia"], ref["inertia"]))


def _same_bits(a, b):
    return a["mass"] == b["mass"] and np.array_equal(a["com"], b["com"]) and np.array_equal(a["second_moment"], b["second_moment"])


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_mass_properties_against_the_closed_forms(key):
    en, pos = DU.mesh_tables(key)
    dim = key[0]
    c = _context(key)
    for name in [None] + DU.FIELDS:
        rho = None if name is None else DU.field(key, name)
        c.set_density(rho)
        got, ref = c.mass_properties(), DU.mass_properties(dim, en, pos, rho)
        err = _props_err(got, ref)
        print("%s %s: mass %.6f, %.3e relative" % (_name(key), name, got["mass"], err))
        assert err <= TOL
        assert _same_bits(got, c.mass_properties())
        twice = c.mass_properties(scale=2.0)                                    # the scalar multiplies mass and moments, not the centre
        assert abs(twice["mass"] / ref["mass"] - 2) <= 2 * TOL and _scale_err(twice["second_moment"], 2 * ref["second_moment"]) <= TOL
        assert np.array_equal(twice["com"], got["com"])
    c.close()


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_mass_properties_far_from_the_origin(key):
    """the same body moved by (1e6, -2e6, 3e6): mass and the second moments about the centre do not change (to the rounding of the moved
    vertices, 1e6 eps of the body's size); a one-pass moment about the origin would lose eight digits"""
    V, T, deg, _ = U.mesh_arrays(key)
    shift = np.array([1e6, -2e6, 3e6])[:V.shape[1]]
    rho = DU.field(key, "bimaterial")
    c = _context(key, field="bimaterial")
    here = c.mass_properties()
    c.mesh_update_vertices(np.ascontiguousarray(V + shift))                     # (the field survives the update)
    there = c.mass_properties()
    c.close()
    em = abs(there["mass"] / here["mass"] - 1)
    es = _scale_err(there["second_moment"], here["second_moment"])
    ec = np.abs(there["com"] - shift - here["com"]).max() / np.abs(here["com"]).max()
    print("%s: mass %.3e, second moments %.3e, centre %.3e" % (_name(key), em, es, ec))
    assert em <= 1e-8 and es <= 1e-8
    assert ec <= 1e-8
    assert rho.max() == 8.0


def test_mass_properties_past_the_grid_cap():
    """a linear tet mesh with more elements than one stride of the capped grid covers: the lanes loop"""
    from meshfem_amd import grid
    per_cell = len(grid.grid_tet_mesh(1, 1, 1)[1])
    n = 1
    while per_cell * n ** 3 <= MASS_GRID_CAP * 256:
        n += 1
    V, T = grid.grid_tet_mesh(n, n, n, [0, 0, 0], [1.0, 1.5, 2.0])
    assert len(T) > MASS_GRID_CAP * 256 and per_cell * (n - 1) ** 3 <= MASS_GRID_CAP * 256
    c = M.Context(0)
    c.mesh_build(T, V, 1)
    rho = np.random.default_rng(2).uniform(0.5, 4.0, len(T))
    c.set_density(rho)
    got, ref = c.mass_properties(), DU.mass_properties(3, c.elem_nodes(), c.node_positions(), rho)
    err = _props_err(got, ref)
    print("%d^3 cells, %d tets: %.3e relative" % (n, len(T), err))
    assert err <= TOL
    assert _same_bits(got, c.mass_properties())
    c.close()


def test_modal_effective_mass_sums_to_the_mass():
    """all modes of the free (3, 1) body, M_rho-orthonormal (dense eigh): X^T X = M^-1, so sum_j (x_j^T M r_d)^2 = r_d^T M r_d = the mass, in
    every direction. Bar: eigh's own orthonormality defect times the number of modes."""
    from meshfem_amd.linear_elasticity import Simulator
    key = (3, 1)
    V, T, deg, _ = U.mesh_arrays(key)
    sim = Simulator(T, V, deg)
    sim.setIsotropicMaterial(U.E_MOD, U.NU)
    sim.setDensity(DU.field(key, "bimaterial"))
    _, X, _, defect = DU.free_truth(key, "bimaterial")
    eff = sim.modalEffectiveMass(X.T)
    mass = sim.massProperties()["mass"]
    assert eff.shape == (X.shape[1], 3) and np.all(eff >= 0)
    err = np.abs(eff.sum(axis=0) / mass - 1).max()
    bar = 10 * X.shape[1] * max(defect, EPS)
    print("effective masses sum to %s of the mass %.6f: %.3e (bar %.3e)" % (eff.sum(axis=0) / mass, mass, err, bar))
    assert err <= bar
    sim.ctx.close()


# ------------------------------------------------------------------------------------------------ 7: state
@pytest.mark.parametrize("key", [(2, 2), (3, 1)], ids=_name)
def test_changing_the_field_between_solves(key):
    a, b = DU.field(key, "bimaterial"), DU.field(key, "random")
    x = _rand(key[0] * len(DU.mesh_tables(key)[1]))
    c = _context(key)
    c.fix_variables(U.clamp_vars(key))
    c.set_density(a)
    lam_a, _, _ = c.modes(4, rtol=1e-9, maxit=5000)
    c.set_density(b)
    lam_b, _, _ = c.modes(4, rtol=1e-9, maxit=5000)
    y_b = c.mass_apply(x)
    fresh = _context(key)
    fresh.fix_variables(U.clamp_vars(key))
    fresh.set_density(b)
    lam_f, _, _ = fresh.modes(4, rtol=1e-9, maxit=5000)
    y_f = fresh.mass_apply(x)
    fresh.close()
    print("%s: second field against a fresh context: lambda %.3e, M x %.3e of scale" % (_name(key), np.abs(lam_b / lam_f - 1).max(), _scale_err(y_b, y_f)))
    assert np.abs(lam_a / lam_b - 1).max() > 1e-3                               # the two fields are different bodies
    assert np.abs(lam_b / lam_f - 1).max() <= 1e-10
    assert _scale_err(y_b, y_f) <= 1e-14
    # a vertex update keeps the field
    V, T, deg, _ = U.mesh_arrays(key)
    V2 = V * 1.25
    c.mesh_update_vertices(np.ascontiguousarray(V2))
    en, pos = c.elem_nodes(), c.node_positions()
    assert _scale_err(c.mass_apply(x), DU.mass_matrix(key[0], deg, en, pos, b) @ x) <= TOL
    # None restores unit density
    c.set_density(None)
    assert _scale_err(c.mass_apply(x), DU.mass_matrix(key[0], deg, en, pos) @ x) <= TOL
    # a new mesh clears the field
    c.set_density(b)
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    assert _scale_err(c.mass_apply(x), DU.M_rho(key) @ x) <= TOL
    assert abs(c.mass_properties()["mass"] / DU.mass_properties(key[0], *DU.mesh_tables(key))["mass"] - 1) <= TOL
    c.close()


@pytest.mark.parametrize("deterministic", [1, 0])
@pytest.mark.parametrize("key", [(2, 2), (3, 2)], ids=_name)
def test_two_contexts_with_the_same_field(key, deterministic):
    """under option deterministic the assembly adds in a fixed order: the same bits; without it the LDS adds of a slot meet in any order: 1e-14"""
    x = _rand(key[0] * len(DU.mesh_tables(key)[1]))
    ys = []
    for _ in range(2):
        c = _context(key, options=(("deterministic", deterministic),), field="random")
        ys.append(c.mass_apply(x))
        c.close()
    if deterministic:
        assert np.array_equal(ys[0], ys[1])
    assert _scale_err(ys[0], ys[1]) <= 1e-14
    assert _scale_err(ys[0], DU.M_rho(key, "random") @ x) <= TOL


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_refusals():
    key = (2, 1)
    c = _context(key)
    c.fix_variables(U.clamp_vars(key))
    n_elem = c.n_elem
    good = DU.field(key, "random")
    c.set_density(good)
    x = _rand(c.dim * c.n_dof)
    before = c.mass_apply(x)
    lib = c.lib
    ref = DU.clamped_truth(key, "random")

    def refused(status, code=L.ERR_INVALID):
        """the call was refused with `code`, the field in force is untouched and the context still solves"""
        assert status == code
        assert _scale_err(c.mass_apply(x), before) <= 1e-14
        lam, _, info = c.modes(1, rtol=RTOL, maxit=3000)
        assert info["converged"] == 1 and abs(lam[0] - ref[0][0]) <= np.sqrt(ref[2]) * RTOL * ref[0][0]
    d = _Dev(c)
    try:
        bads = []
        for v in (0.0, -1.0, np.nan, np.inf):
            bad = np.array(good)
            bad[n_elem // 2] = v
            bads.append(bad)
        for bad in bads:
            refused(lib.mfh_set_density(c.h, ptr(bad), n_elem, 0))
            refused(lib.mfh_set_density(c.h, d.up(bad), n_elem, L.LOAD_ON_DEVICE))
        for n in (n_elem - 1, n_elem + 1, 0):
            refused(lib.mfh_set_density(c.h, ptr(good), n, 0))
            refused(lib.mfh_set_density(c.h, d.up(good), n, L.LOAD_ON_DEVICE))
        refused(lib.mfh_set_density(c.h, ptr(good), n_elem, 4))
        y = np.empty_like(before)
        refused(lib.mfh_mass_apply(c.h, None, ptr(y), 0))
        refused(lib.mfh_mass_apply(c.h, ptr(x), ptr(y), 1))
        mass = C.c_double()
        refused(lib.mfh_mass_properties(c.h, 0.0, C.byref(mass), None, None, 0))
        refused(lib.mfh_mass_properties(c.h, 1.0, C.byref(mass), None, None, 2))
        with pytest.raises(ValueError):
            c.mass_apply(x[:-1])
    finally:
        d.free()
    c.close()
    # MFH_ERR_STATE: no mesh; a matrix from mfh_matrix_set_upper_triplets; a host-only context
    one = np.ones(4)
    e = M.Context(0)
    mass = C.c_double()
    assert e.lib.mfh_set_density(e.h, ptr(one), 4, 0) == L.ERR_STATE
    assert e.lib.mfh_mass_properties(e.h, 1.0, C.byref(mass), None, None, 0) == L.ERR_STATE
    assert e.lib.mfh_mass_apply(e.h, ptr(one), ptr(one.copy()), 0) == L.ERR_STATE
    e.matrix_set_upper_triplets(3, [0, 1, 2], [0, 1, 2], [1.0, 2.0, 3.0])
    assert e.lib.mfh_set_density(e.h, ptr(one), 4, 0) == L.ERR_STATE
    assert e.lib.mfh_mass_properties(e.h, 1.0, C.byref(mass), None, None, 0) == L.ERR_STATE
    assert e.lib.mfh_mass_apply(e.h, ptr(one), ptr(one.copy()), 0) == L.ERR_STATE
    e.close()
    V, T, deg, _ = U.mesh_arrays(key)
    h = M.Context(-1)
    h.mesh_build(T, V, deg)
    assert h.lib.mfh_set_density(h.h, ptr(good), n_elem, 0) == L.ERR_STATE
    assert h.lib.mfh_mass_properties(h.h, 1.0, C.byref(mass), None, None, 0) == L.ERR_STATE
    h.close()
    # MFH_ERR_UNSUPPORTED: a row-partitioned context
    p = M.Context(0)
    p.mesh_set(2, 1, T, V, n_owned=len(V) - 3)
    p.material_isotropic(U.E_MOD, U.NU)
    assert p.lib.mfh_set_density(p.h, ptr(good), n_elem, 0) == L.ERR_UNSUPPORTED
    assert p.lib.mfh_set_density(p.h, None, 0, 0) == L.ERR_UNSUPPORTED
    assert p.lib.mfh_mass_properties(p.h, 1.0, C.byref(mass), None, None, 0) == L.ERR_UNSUPPORTED
    assert p.lib.mfh_mass_apply(p.h, ptr(np.ones(2 * len(V))), ptr(np.ones(2 * len(V))), 0) == L.ERR_UNSUPPORTED
    p.close()


def test_simulator_layer():
    """an array-valued density= of vibrational_modes / transient sets the field and passes the scalar 1"""
    from meshfem_amd.linear_elasticity import Simulator
    key = (3, 1)
    V, T, deg, V0 = U.mesh_arrays(key)
    sim = Simulator(T, V, deg)
    sim.setIsotropicMaterial(U.E_MOD, U.NU)
    rho = DU.field(key, "bimaterial")
    freq, shapes = sim.vibrational_modes(3, density=rho, free=True)
    nz = 6
    ref, _, cond, _ = DU.free_truth(key, "bimaterial")
    lam = (2.0 * np.pi * freq) ** 2
    assert np.all(np.abs(lam - ref[nz:nz + 3]) <= np.sqrt(cond) * RTOL * ref[nz:nz + 3])
    x = _rand((sim.numDoFs(), 3))
    assert _scale_err(sim.applyMassMatrix(x).ravel(), DU.M_rho(key, "bimaterial") @ x.ravel()) <= TOL        # the field stayed in force
    eff = sim.modalEffectiveMass(shapes)
    assert eff.shape == (3, 3) and np.all(eff <= 1e-12 * sim.massProperties()["mass"])      # free modes carry no net momentum
    with pytest.raises(ValueError):
        sim.vibrational_modes(3, density=rho[:-1], free=True)
    r = sim.transient(0.1, 3, v0=np.ones((sim.numNodes(), 3)), density=2.0 * rho, energies=True)
    assert abs(r["energies"][0, 0] / (0.5 * 3 * sim.massProperties()["mass"]) - 1) <= 1e-12    # 1/2 v.Mv of the unit velocity in all three directions; the field in force is 2 rho
    sim.ctx.close()
