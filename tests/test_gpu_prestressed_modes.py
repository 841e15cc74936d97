"""Prestressed vibration on the device (mfh_modes_prestressed, mfh_tangent_apply, the pair product k_spmv_kron_pair;
docs/design/04_18_prestressed_modes.md) against the dense truth of tests/prestress_util.py, which tests/test_prestressed_modes_reference.py pins
on the CPU. Meshes: the four column fixtures of buckling_util (about 1 700 unknowns and fewer) under unit axial compression, at -1, 0.5, 0.9 and
1.1 of their critical factor; the mid mesh of modes_util (several row chunks) for the pair product. rtol = 1e-6, maxit = 3000 throughout.
Bars:
  pair product   componentwise: |yA - (yA0 + s Kg x)|_r <= |s| (N_r + 40) eps sum_j |Kg|_rj |x_j| + the two single roundings of the scaling and the
                 sum; |yB - rho M x|_r alike with |M| (buckling_util.product_bound, prestress_util.mass_product_bound / pair_bounds) -- the
                 worst-case rounding bounds of the sums in any order, for the single pass and for the two-launch form
  tangent        the same bar with yA0 = the device's own K x (mfh_apply_K runs the same operator launch; K x against the oracle is the subject
                 of tests/test_gpu_parity.py)
  eigenvalues    |lambda~ - lambda| <= sqrt(cond2(M_ff)) rtol |lambda|: the first-order residual bound of tests/test_gpu_modes.py
  residuals      recomputed on the host from the exported K, the numpy Kg and M: <= 2 rtol
  orthonormality ||X M X^T - I||_max <= max(10 x the defect of eigh's own eigenvectors on the case, n eps): the bar of tests/test_gpu_modes.py
Every solve is made once (functools.lru_cache) and shared by the tests that look at it."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import meshfem_amd as M
from meshfem_amd import _lib as L
from meshfem_amd._lib import ptr

import buckling_util as B
import density_util as D
import modes_util as U
import prestress_util as P

pytestmark = pytest.mark.gpu

RTOL = 1e-6
MAXIT = 3000
NEV = 4
EPS = U.EPS
PRECONDS = {"jacobi": M.PRECOND_BLOCK_JACOBI, "two-level": M.PRECOND_TWO_LEVEL, "multigrid": M.PRECOND_MULTIGRID}


def _name(key):
    return key if isinstance(key, str) else "%dD-P%d" % key


def _context(key, precond="jacobi", options=()):
    V, T, deg, _ = B.mesh_arrays(key)
    c = M.Context(0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    c.set_preconditioner(PRECONDS[precond])
    return c


def _rand(n, seed=5):
    return np.random.default_rng(seed).standard_normal(n)


def _sigma(key, seed=3):
    en, pos = B.mesh_tables(key)
    return B.random_symmetric_field(len(en), pos.shape[1], seed)


def _clamp(key):
    return B.clamp_vars(key)


def _check(tag, got, ref, bar):
    err = np.abs(np.asarray(got).ravel() - np.asarray(ref).ravel())
    bar = np.asarray(bar).ravel()
    print("%s: max error / bar %.3e (max error %.3e of scale)" % (tag, (err / np.maximum(bar, 1e-300)).max(), err.max() / max(np.abs(ref).max(), 1e-300)))
    assert np.all(np.isfinite(got)) and np.all(err <= bar)


# ------------------------------------------------------------------------------------------------ the pair product
def _pair_reference(dim, deg, en, pos, sig, rho_field, s, rho, x, yA0, fixed=None, dof=None, n_dof=None):
    """(ref_A, ref_B, bar_A, bar_B) of yA0 + s Kg x and rho M x in numpy; rows of `fixed` are zero in both, exactly"""
    Kg = B.geometric_stiffness(dim, deg, en, pos, sig, dof, n_dof)
    Mm = D.mass_matrix(dim, deg, en, pos, rho_field, dof, n_dof)
    gx, mx = Kg @ x, Mm @ x
    bg = B.product_bound(dim, deg, en, pos, sig, x.reshape(-1, dim), dof, n_dof).ravel()
    bm = P.mass_product_bound(dim, deg, en, pos, rho_field, x.reshape(-1, dim), dof, n_dof).ravel()
    bar_A, bar_B = P.pair_bounds(s, rho, yA0, gx, mx, bg, bm)
    ref_A, ref_B = yA0 + s * gx, rho * mx
    if fixed is not None:
        for a in (ref_A, ref_B, bar_A, bar_B):
            a[fixed] = 0.0
    return ref_A, ref_B, bar_A, bar_B


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("key", P.COLUMNS + [U.MID], ids=_name)
def test_pair_product_against_numpy(key, masked):
    """a random symmetric prestress, a non-unit density field and a scalar density on top of it, yA pre-filled with a random vector; the single
    pass and the forced two-launch form both meet the bar, and their yA agree to the last bit: the kernel rounds where the two launches round,
    and Kg is always assembled in a fixed order (yB: test_pair_product_repeats_bit_for_bit, on contexts whose mass buffer is too)"""
    c = _context(key)
    en, pos = B.mesh_tables(key)
    assert np.array_equal(c.node_positions(), pos) and np.array_equal(c.elem_nodes(), en)      # the oracle's numbering is the library's own
    dim, deg = pos.shape[1], B.mesh_arrays(key)[2]
    n = dim * c.n_dof
    x, yA0 = _rand(n), _rand(n, 6)
    sig = _sigma(key)
    rho_field = D.density_field("random", en, pos, dim)
    s, rho = -0.37, 2.5
    fixed = _clamp(key) if masked else None
    if masked:
        c.fix_variables(fixed)
    c.set_prestress(sig)
    c.set_density(rho_field)
    ref_A, ref_B, bar_A, bar_B = _pair_reference(dim, deg, en, pos, sig, rho_field, s, rho, x, yA0, fixed)
    out = {}
    for two_pass in (False, True):
        tag = "%s %s" % (_name(key), "two launches" if two_pass else "single pass")
        a, b = c.debug_kron_pair(s, rho, x, yA0, masked=masked, two_pass=two_pass)
        _check(tag + " yA", a, ref_A, bar_A)
        _check(tag + " yB", b, ref_B, bar_B)
        if masked:
            assert np.all(a[fixed] == 0.0) and np.all(b[fixed] == 0.0)
        out[two_pass] = (a, b)
    assert np.array_equal(out[False][0], out[True][0])
    a, _ = c.debug_kron_pair(0.0, 1.0, x, yA0, masked=False)      # s = 0: yA comes back as it went in
    assert np.array_equal(a, yA0)
    c.close()


def test_pair_product_under_a_periodic_dof_map():
    """the unit cell with its interior perturbed, quadratic triangles: P^T Kg P and P^T M P"""
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
    sig = B.random_symmetric_field(len(en), 2)
    rho_field = D.density_field("random", en, pos, 2)
    c.set_prestress(sig)
    c.set_density(rho_field)
    x, yA0 = _rand(2 * n_dof), _rand(2 * n_dof, 6)
    s, rho = 1.75, 0.5
    ref_A, ref_B, bar_A, bar_B = _pair_reference(2, 2, en, pos, sig, rho_field, s, rho, x, yA0, None, dof, n_dof)
    for two_pass in (False, True):
        a, b = c.debug_kron_pair(s, rho, x, yA0, masked=False, two_pass=two_pass)
        _check("periodic 2D-P2 yA (two_pass %d)" % two_pass, a, ref_A, bar_A)
        _check("periodic 2D-P2 yB (two_pass %d)" % two_pass, b, ref_B, bar_B)
    c.close()


@pytest.mark.parametrize("key,options", [("strip-P1", (("deterministic", 1),)), ("col3d-P2", (("deterministic", 1),)), ("col3d-P2", (("matrix_storage", 0),)),
                                         (U.MID, (("deterministic", 1),))],
                         ids=["strip-P1-deterministic", "col3d-P2-deterministic", "col3d-P2-both-triangles", "mid-deterministic"])
def test_pair_product_repeats_bit_for_bit(key, options):
    """Each form returns the same bits in two calls on one context -- the same bits in both forms -- and (option deterministic: the mass buffer is then assembled by the turn-taking
    flavour, like Kg always is) on a fresh context. Without that option the default quadratic context reassembles M in arrival order in every call
    that widened its pattern; with both triangles stored it is assembled once."""
    dim = B.mesh_tables(key)[1].shape[1]
    n = dim * len(B.mesh_tables(key)[1])
    x, yA0 = _rand(n), _rand(n, 6)

    def run(c, two_pass):
        return c.debug_kron_pair(0.8, 1.5, x, yA0, masked=True, two_pass=two_pass)

    def fresh():
        c = _context(key, options=options)
        c.fix_variables(_clamp(key))
        c.set_prestress(_sigma(key))
        return c
    c = fresh()
    first = {tp: run(c, tp) for tp in (False, True)}
    for tp in (False, True):
        again = run(c, tp)
        assert np.array_equal(first[tp][0], again[0]) and np.array_equal(first[tp][1], again[1])
    assert np.array_equal(first[False][0], first[True][0]) and np.array_equal(first[False][1], first[True][1])
    c.close()
    if ("deterministic", 1) in options:
        f = fresh()
        for tp in (False, True):
            other = run(f, tp)
            assert np.array_equal(first[tp][0], other[0]) and np.array_equal(first[tp][1], other[1])
        f.close()


# ------------------------------------------------------------------------------------------------ the tangent product
@pytest.mark.parametrize("key", P.COLUMNS + [U.MID], ids=_name)
def test_tangent_apply(key):
    c = _context(key, options=(("deterministic", 1),))          # (the K part is then the same bits in every call)
    en, pos = B.mesh_tables(key)
    dim, deg = pos.shape[1], B.mesh_arrays(key)[2]
    x = _rand(dim * c.n_dof)
    sig = _sigma(key)
    c.fix_variables(_clamp(key))                                  # no effect: the product is unmasked
    c.set_prestress(sig)
    kx = c.apply_K(x)
    gx = B.geometric_stiffness(dim, deg, en, pos, sig) @ x
    bg = B.product_bound(dim, deg, en, pos, sig, x.reshape(-1, dim)).ravel()
    for s in (0.6, -3.0):
        bar, _ = P.pair_bounds(s, 1.0, kx, gx, 0 * gx, bg, 0 * bg)
        _check("%s s = %g" % (_name(key), s), c.tangent_apply(x, s), kx + s * gx, bar)
    _check("%s s = 0" % _name(key), c.tangent_apply(x, 0.0), kx, P.pair_bounds(0.0, 1.0, kx, gx, 0 * gx, bg, 0 * bg)[0])
    # against the oracle's K as well, on the scale of the product (the bar of tests/test_gpu_parity.py for K x, plus Kg's componentwise one)
    if key != U.MID:
        ref = B.stiffness(key) @ x + 0.6 * gx
        err = np.abs(c.tangent_apply(x, 0.6) - ref)
        assert np.all(err <= 1e-13 * np.abs(ref).max() + 0.6 * bg + 2 * EPS * np.abs(ref))
        d = _dev(c)                                               # device pointers
        try:
            y = d.alloc(8 * x.size)
            c._ck(c.lib.mfh_tangent_apply(c.h, 0.6, d.up(x), y, L.LOAD_ON_DEVICE))
            assert np.array_equal(d.down(y, x.shape), c.tangent_apply(x, 0.6))
        finally:
            d.free()
    c.close()


class _dev:
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


# ------------------------------------------------------------------------------------------------ eigenvalues
@functools.lru_cache(maxsize=None)
def _solve(key, precond, ratio):
    c = _context(key, precond)
    assert np.array_equal(c.node_positions(), B.mesh_tables(key)[1])
    c.fix_variables(_clamp(key))
    c.set_prestress(B.axial_compression(key))
    lam, X, info = c.modes_prestressed(NEV, ratio * P.critical_factor(key), rtol=RTOL, maxit=MAXIT)
    c.close()
    return lam, X, info


CASES = [(k, "jacobi", r) for k in P.COLUMNS for r in P.FACTORS] + \
        [(k, p, r) for k in ("col3d-P2", "strip-P1") for p in ("two-level", "multigrid") for r in P.FACTORS]


@pytest.mark.parametrize("key,precond,ratio", CASES, ids=lambda v: str(v))
def test_eigenvalues_against_dense_truth(key, precond, ratio):
    lam, X, info = _solve(key, precond, ratio)
    ref = P.truth(key, ratio)[0][:NEV]
    bar = np.sqrt(P.cond_of_mass(key)) * RTOL * np.abs(ref)
    err = np.abs(lam - ref)
    print("%s %s at %.1f of the critical factor: %d unknowns, %d iterations, block %d, restarts %d, precondUsed %d, lambda %s, max err / bar %.3e, note '%s'" %
          (key, precond, ratio, len(B.free_vars(key)), info["iterations"], info["blockSize"], info["restarts"], info["precondUsed"], lam, (err / bar).max(), info["note"]))
    assert info["converged"] == 1 and info["maxResidual"] <= RTOL
    assert np.all(np.diff(lam) >= 0)
    assert np.all(err <= bar)
    if ratio > 1.0:
        assert lam[0] < 0 < lam[1] and "1 of the %d eigenvalues are negative" % NEV in info["note"] and "unstable" in info["note"]
    else:
        assert np.all(lam > 0) and "negative" not in info["note"]


@functools.lru_cache(maxsize=None)
def _device_K(key):
    c = _context(key)
    n = c.bs * c.n_dof
    c.assemble()
    i, j, v = c.export_upper_triplets()
    c.close()
    U_ = sp.coo_matrix((v, (i.astype(np.int64), j.astype(np.int64))), shape=(n, n)).tocsr()
    return sp.csr_matrix(U_ + sp.triu(U_, 1).T)


@pytest.mark.parametrize("key,precond,ratio", CASES, ids=lambda v: str(v))
def test_residuals_orthonormality_clamp_and_sign(key, precond, ratio):
    lam, X, info = _solve(key, precond, ratio)
    f = B.free_vars(key)
    s = ratio * P.critical_factor(key)
    A = _device_K(key) + s * B.Kg_of(key, B.axial_compression(key))
    Mm = P.mass(key)
    res = P.host_residuals(A[f][:, f], Mm[f][:, f], lam, X[:, f])
    n = X.shape[1]
    defect = np.abs(X @ (Mm @ X.T) - np.eye(len(X))).max()
    defect_ref = P.truth(key, ratio)[2]
    print("%s %s at %.1f: residuals recomputed %s reported %s; defect %.3e, eigh's %.3e, n eps %.3e" %
          (key, precond, ratio, res, info["residuals"], defect, defect_ref, n * EPS))
    assert np.all(res <= 2 * RTOL)
    assert defect <= max(10 * defect_ref, n * EPS)
    assert np.all(X[:, _clamp(key)] == 0.0)
    assert U.sign_rule_holds(X)


# ------------------------------------------------------------------------------------------------ agreement with the existing entry points
@pytest.mark.parametrize("key", ["col3d-P2", "strip-P1"])
def test_agreement_with_modes_and_buckling(key):
    """s = 0 is Context.modes (each side carries the eigenvalue bar); with the critical factor taken from Context.buckling on the SAME context the
    first eigenvalue is positive at 0.9 of it and negative at 1.1"""
    c = _context(key)
    c.fix_variables(_clamp(key))
    c.set_prestress(B.axial_compression(key))
    lam0, _, _ = c.modes_prestressed(NEV, 0.0, rtol=RTOL, maxit=MAXIT)
    lam, _, _ = c.modes(NEV, rtol=RTOL, maxit=MAXIT)
    bar = np.sqrt(P.cond_of_mass(key)) * RTOL * np.abs(lam)
    print("%s: |lambda(s = 0) - lambda(modes)| / bar %s" % (key, np.abs(lam0 - lam) / bar))
    assert np.all(np.abs(lam0 - lam) <= 2 * bar)
    cr = c.buckling(1, rtol=RTOL, maxit=MAXIT)[0][0]
    below = c.modes_prestressed(1, 0.9 * cr, rtol=RTOL, maxit=MAXIT)[0][0]
    above = c.modes_prestressed(1, 1.1 * cr, rtol=RTOL, maxit=MAXIT)[0][0]
    print("%s: critical factor %.6g (truth %.6g), lambda_1 %.4e at 0.9, %.4e at 1.1" % (key, cr, P.critical_factor(key), below, above))
    assert below > 0 > above
    c.close()


def test_warm_start():
    """started from the converged shapes at 0.5 of the critical factor, the call at 0.55 takes no more iterations than the cold one, and returns the
    same eigenvalues within the bar on each side"""
    key = "col3d-P1"
    cr = P.critical_factor(key)
    _, X5, _ = _solve(key, "jacobi", 0.5)
    c = _context(key)
    c.fix_variables(_clamp(key))
    c.set_prestress(B.axial_compression(key))
    cold, _, ic = c.modes_prestressed(NEV, 0.55 * cr, rtol=RTOL, maxit=MAXIT)
    warm, _, iw = c.modes_prestressed(NEV, 0.55 * cr, x0=X5, rtol=RTOL, maxit=MAXIT)
    print("warm start on %s: %d iterations cold, %d started from the shapes at 0.5" % (key, ic["iterations"], iw["iterations"]))
    assert iw["iterations"] <= ic["iterations"]
    assert np.all(np.abs(warm - cold) <= 2 * np.sqrt(P.cond_of_mass(key)) * RTOL * np.abs(cold))
    c.close()


# ------------------------------------------------------------------------------------------------ the Simulator layer
def test_simulator_prestressed_modes():
    """Simulator.prestressedModes on the linear column pushed down by a traction on its top face: the chain done by hand on the same context gives
    the same bits (option deterministic), doubling the load and halving the factors the same eigenvalues (the bar on each side), and factor 0 the
    frequencies of vibrational_modes"""
    from meshfem_amd.linear_elasticity import Simulator
    key = "col3d-P1"
    V, T, deg, _ = B.mesh_arrays(key)
    sim = Simulator(T, V, deg)
    sim.ctx.set_option("deterministic", 1)
    sim.rtol = 1e-11
    sim.setIsotropicMaterial(U.E_MOD, U.NU)
    nodes = np.unique(_clamp(key) // 3)
    sim.applyDirichletNodes(nodes, np.zeros((len(nodes), 3)))
    sim.applyNeumannBox([-0.01, -0.01, 0.985], [1.01, 1.01, 1.01], [0, 0, -1.0], relative=True)
    load = sim.neumannLoad()
    cr = sim.buckling(1, maxit=MAXIT)[0][0]
    factors = (0.5 * cr, 0.55 * cr)
    lam, modes, u = sim.prestressedModes(NEV, factors=factors, maxit=MAXIT)
    infos = sim.prestressed_modes_info
    assert lam.shape == (2, NEV) and modes.shape == (2, NEV, sim.numNodes(), 3) and u.shape == (sim.numNodes(), 3)
    assert all(i["converged"] == 1 for i in infos) and np.all(lam > 0) and lam[1, 0] < lam[0, 0]
    print("Simulator: critical factor %.6g, lambda %s -> %s, iterations %d -> %d (warm)" % (cr, lam[0], lam[1], infos[0]["iterations"], infos[1]["iterations"]))
    # by hand
    ctx = sim.ctx
    uh = sim.solve()
    ctx.prestress_from_displacement(uh)
    v, _ = ctx.bc_dirichlet_vars()
    ctx.clear_fixed()
    ctx.fix_variables(v)
    l1, X1, _ = ctx.modes_prestressed(NEV, factors[0], rtol=1e-6, maxit=MAXIT)
    l2, X2, _ = ctx.modes_prestressed(NEV, factors[1], x0=X1, rtol=1e-6, maxit=MAXIT)
    assert np.array_equal(u, uh)
    assert np.array_equal(lam[0], l1) and np.array_equal(lam[1], l2)
    assert np.array_equal(modes[0].reshape(NEV, -1), X1) and np.array_equal(modes[1].reshape(NEV, -1), X2)
    # (load x 2, factors / 2)
    bar = np.sqrt(P.cond_of_mass(key)) * RTOL * np.abs(lam)
    lam2, _, _ = sim.prestressedModes(NEV, load=2.0 * load, factors=[0.5 * s for s in factors], maxit=MAXIT)
    print("Simulator: |lambda(2 load, s / 2) - lambda(load, s)| / bar %s" % (np.abs(lam2 - lam) / bar))
    assert np.all(np.abs(lam2 - lam) <= 2 * bar)
    # factor 0
    lam0, _, _ = sim.prestressedModes(NEV, factors=(0.0,), maxit=MAXIT)
    freq, _ = sim.vibrational_modes(NEV, maxit=MAXIT)
    want = (2 * np.pi * freq) ** 2
    assert np.all(np.abs(lam0[0] - want) <= 2 * np.sqrt(P.cond_of_mass(key)) * RTOL * want)
    sim.ctx.close()


# ------------------------------------------------------------------------------------------------ state
def _probe(c):
    n = c.bs * c.n_dof
    rng = np.random.default_rng(5)
    f, x = rng.standard_normal(n), rng.standard_normal(n)
    u = c.solve(f, rtol=1e-9)
    return u, c.apply_K(x), c.geometric_apply(x), c.modes(3, rtol=RTOL)[:2], c.buckling(3, rtol=RTOL, maxit=MAXIT)[:2]


@pytest.mark.parametrize("storage", [-1, 0], ids=["default-storage", "both-triangles"])
def test_nothing_existing_moves(storage):
    """A context that has run mfh_modes_prestressed and mfh_tangent_apply solves, applies K and Kg and computes its vibrational and buckling modes
    like a fresh one, bit for bit -- also the default quadratic context, whose pattern the calls widened for their own duration (both contexts
    with option deterministic 1, as in tests/test_gpu_modes.py). Two prestressed calls give the same bits."""
    key = (3, 2)
    opts = (("deterministic", 1), ("matrix_storage", storage))
    fixed = U.clamp_vars(key)
    en, _ = B.mesh_tables(key)
    S = np.zeros((3, 3))
    S[0, 0] = -1.0                                        # compression along x, the axis the clamp is normal to
    sig = B.uniform_field(len(en), 3, S)
    a = _context(key, "multigrid", opts)
    a.fix_variables(fixed)
    a.set_prestress(sig)
    lam, X, info = a.modes_prestressed(3, 0.01, rtol=RTOL, maxit=MAXIT)
    assert info["converged"] == 1 and ("both triangles" in info["note"]) == (storage == -1)
    a.tangent_apply(_rand(3 * a.n_dof), 0.01)
    got = _probe(a)
    b = _context(key, "multigrid", opts)
    b.fix_variables(fixed)
    b.set_prestress(sig)
    want = _probe(b)
    for g, w_ in zip(got[:3], want[:3]):
        assert np.array_equal(g, w_)
    for g, w_ in zip(got[3] + got[4], want[3] + want[4]):
        assert np.array_equal(g, w_)
    lam2, X2, _ = a.modes_prestressed(3, 0.01, rtol=RTOL, maxit=MAXIT)
    assert np.array_equal(lam, lam2) and np.array_equal(X, X2)
    a.close(); b.close()


def test_prestress_and_density_take_effect():
    key = "strip-P2"
    cr = P.critical_factor(key)
    bar = 2 * np.sqrt(P.cond_of_mass(key)) * RTOL
    c = _context(key)
    c.fix_variables(_clamp(key))
    c.set_prestress(B.axial_compression(key))
    ref = P.truth(key, 0.5)[0][:NEV]
    lam = c.modes_prestressed(NEV, 0.5 * cr, rtol=RTOL, maxit=MAXIT)[0]
    assert np.all(np.abs(lam - ref) <= bar * ref)
    c.set_prestress(B.axial_compression(key, 2.0))         # twice the stress: the spectrum of 0.9 at 0.45 ...
    ref9 = P.truth(key, 0.9)[0][:NEV]
    lam = c.modes_prestressed(NEV, 0.45 * cr, rtol=RTOL, maxit=MAXIT)[0]
    assert np.all(np.abs(lam - ref9) <= bar * ref9)
    lam = c.modes_prestressed(NEV, 0.25 * cr, rtol=RTOL, maxit=MAXIT)[0]      # ... and that of 0.5 at 0.25
    assert np.all(np.abs(lam - ref) <= bar * ref)
    lam = c.modes_prestressed(NEV, 0.25 * cr, density=4.0, rtol=RTOL, maxit=MAXIT)[0]
    assert np.all(np.abs(4.0 * lam - ref) <= bar * ref)
    c.set_density(np.full(c.n_elem, 2.0))                  # the field and the scalar multiply
    lam = c.modes_prestressed(NEV, 0.25 * cr, density=2.0, rtol=RTOL, maxit=MAXIT)[0]
    assert np.all(np.abs(4.0 * lam - ref) <= bar * ref)
    c.set_density(None)
    lam = c.modes_prestressed(NEV, 0.25 * cr, rtol=RTOL, maxit=MAXIT)[0]
    assert np.all(np.abs(lam - ref) <= bar * ref)
    c.close()


def test_maxit_two():
    key = "col3d-P2"
    c = _context(key)
    c.fix_variables(_clamp(key))
    c.set_prestress(B.axial_compression(key))
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes_prestressed(NEV, 0.5 * P.critical_factor(key), rtol=RTOL, maxit=2)
    assert ei.value.code == L.ERR_NOT_CONVERGED
    lam, X, info = c.last_modes_prestressed
    assert info["iterations"] == 2 and info["converged"] == 0
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(X)) and np.all(np.diff(lam) >= 0) and np.all(lam > 0)
    u = c.solve(np.ones(c.bs * c.n_dof), rtol=1e-8)
    assert c.last_info["converged"] == 1 and np.all(np.isfinite(u))
    c.close()


def test_refusals():
    key = (2, 1)
    c = _context(key)
    c.fix_variables(U.clamp_vars(key))
    c.set_prestress(_sigma(key))
    n = c.dim * c.n_dof
    x = _rand(n)
    before = c.tangent_apply(x, 0.3)
    lib = c.lib
    lam, X, res = np.zeros(21), np.zeros((21, n)), np.zeros(21)
    info = L.ModesInfo()

    def modes(h, nev=1, density=1.0, s=0.1, flags=0, rtol=RTOL, maxit=100, x0=None):
        return lib.mfh_modes_prestressed(h, nev, density, s, flags, rtol, maxit, x0, ptr(lam), ptr(X), ptr(res), C.byref(info))

    def refused(status, code=L.ERR_INVALID):
        """the call was refused with `code` and the context is left usable, its prestress in force"""
        assert status == code
        assert np.abs(c.tangent_apply(x, 0.3) - before).max() <= 1e-14 * np.abs(before).max()
    for nev in (0, 21, -1):
        refused(modes(c.h, nev=nev))
    for s in (np.nan, np.inf, -np.inf):
        refused(modes(c.h, s=s))
        refused(lib.mfh_tangent_apply(c.h, s, ptr(x), ptr(np.empty(n)), 0))
    for rho in (0.0, -1.0, np.nan, np.inf):
        refused(modes(c.h, density=rho))
    refused(modes(c.h, rtol=0.0))
    refused(modes(c.h, maxit=0))
    bad = np.zeros((1, n))
    bad[0, 3] = np.nan
    refused(modes(c.h, x0=ptr(bad)))
    refused(lib.mfh_modes_prestressed(c.h, 1, 1.0, 0.1, 0, RTOL, 100, None, None, ptr(X), ptr(res), C.byref(info)))
    refused(modes(c.h, flags=L.MODES_FREE), L.ERR_UNSUPPORTED)
    assert "rigid rotations are not in the kernel of Kg" in lib.mfh_last_error(c.h).decode()
    refused(modes(c.h, flags=2), L.ERR_UNSUPPORTED)
    y = np.empty(n)
    refused(lib.mfh_tangent_apply(c.h, 0.3, None, ptr(y), 0))
    for flags in (1, 4):                                  # (2 is MFH_LOAD_ON_DEVICE)
        refused(lib.mfh_tangent_apply(c.h, 0.3, ptr(x), ptr(y), flags))
    with pytest.raises(ValueError):
        c.tangent_apply(x[:-1], 0.3)
    with pytest.raises(ValueError):
        c.modes_prestressed(2, 0.1, x0=np.zeros((1, n)))
    # a clamp that leaves rigid motions free; no clamp
    c.clear_fixed()
    c.fix_variables([0, 1])
    refused(modes(c.h), L.ERR_UNSUPPORTED)
    c.clear_fixed()
    refused(modes(c.h), L.ERR_UNSUPPORTED)
    # more modes than the pencil has: all but two variables fixed
    c.fix_variables(np.arange(n - 2))
    refused(modes(c.h, nev=3))
    c.clear_fixed()
    c.fix_variables(U.clamp_vars(key))
    # an operator other than elasticity
    c.set_operator(M.OP_LAPLACIAN)
    assert modes(c.h) == L.ERR_UNSUPPORTED
    assert lib.mfh_tangent_apply(c.h, 0.3, ptr(x), ptr(y), 0) == L.ERR_UNSUPPORTED
    c.set_operator(M.OP_ELASTICITY)
    c.fix_variables(U.clamp_vars(key))
    assert np.abs(c.tangent_apply(x, 0.3) - before).max() <= 1e-14 * np.abs(before).max()
    assert modes(c.h, nev=2, maxit=MAXIT) == L.OK and info.converged == 1
    # no prestress
    c.set_prestress(None)
    assert modes(c.h) == L.ERR_STATE
    assert lib.mfh_tangent_apply(c.h, 0.3, ptr(x), ptr(y), 0) == L.ERR_STATE
    c.close()
    # the forced-degree-1 view
    q = _context((2, 2))
    q.set_prestress(_sigma((2, 2)))
    q.set_operator(M.OP_LAPLACIAN)
    q.set_operator_degree(1)
    xq = np.zeros(2 * q._n_dof_full)
    assert lib.mfh_modes_prestressed(q.h, 1, 1.0, 0.1, 0, RTOL, 100, None, ptr(lam), ptr(np.zeros((1, xq.size))), ptr(res), C.byref(info)) == L.ERR_UNSUPPORTED
    assert lib.mfh_tangent_apply(q.h, 0.3, ptr(xq), ptr(xq.copy()), 0) == L.ERR_UNSUPPORTED
    q.close()
    # MFH_ERR_STATE: no mesh; a matrix from mfh_matrix_set_upper_triplets; a host-only context
    one = np.ones(6)
    e = M.Context(0)
    assert modes(e.h) == L.ERR_STATE
    assert lib.mfh_tangent_apply(e.h, 0.3, ptr(one), ptr(one.copy()), 0) == L.ERR_STATE
    e.matrix_set_upper_triplets(3, [0, 1, 2], [0, 1, 2], [1.0, 2.0, 3.0])
    assert modes(e.h) == L.ERR_STATE
    assert lib.mfh_tangent_apply(e.h, 0.3, ptr(one), ptr(one.copy()), 0) == L.ERR_STATE
    e.close()
    V, T, deg, _ = U.mesh_arrays(key)
    h = M.Context(-1)
    h.mesh_build(T, V, deg)
    assert modes(h.h) == L.ERR_STATE
    assert lib.mfh_tangent_apply(h.h, 0.3, ptr(x), ptr(x.copy()), 0) == L.ERR_STATE
    h.close()
    # MFH_ERR_UNSUPPORTED: a row-partitioned context
    p = M.Context(0)
    p.mesh_set(2, 1, T, V, n_owned=len(V) - 3)
    p.material_isotropic(U.E_MOD, U.NU)
    assert modes(p.h) == L.ERR_UNSUPPORTED
    assert lib.mfh_tangent_apply(p.h, 0.3, ptr(np.ones(2 * len(V))), ptr(np.ones(2 * len(V))), 0) == L.ERR_UNSUPPORTED
    p.close()
