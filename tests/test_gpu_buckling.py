"""Linear buckling on the device (mfh_set_prestress, mfh_prestress_from_displacement, mfh_geometric_apply, mfh_buckling;
docs/design/04_16_buckling.md) against the numpy restatement tests/buckling_util.py, which tests/test_buckling_reference.py pins on the CPU.
Meshes: modes_util.SMALL (the 4 x 3 triangle grid and the 3 x 2 x 2 tet grid, P1 and P2, perturbed), the mid mesh (several row chunks) for the
product; the four column fixtures of buckling_util for the load factors (about 1 000 unknowns and fewer). rtol = 1e-6 throughout.
Bars:
  product        componentwise: |y - Kg x|_r <= (N_r + 40) eps sum_j |Kg|_rj |x_j|, N_r the summands that reach row r, |Kg| with every summand taken by
                 modulus (buckling_util.product_bound) -- the worst-case rounding bound of the sums in any order
  eigenvalues    |mu~ - mu| <= sqrt(cond2(K_ff)) rtol |mu|: the first-order residual bound of tests/test_gpu_modes.py restated for the pencil
                 (Kg, K), whose inner product is K's
  residuals      recomputed on the host from the exported K and the numpy Kg: <= 2 rtol
  orthonormality ||X K X^T - I||_max <= max(10 x the defect of eigh's own eigenvectors on the case, n eps): the bar of tests/test_gpu_modes.py
Every solve is made once (functools.lru_cache) and shared by the tests that look at it."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import meshfem_amd as M
from meshfem_amd import _lib as L
from meshfem_amd._lib import ptr

import buckling_util as B
import modes_util as U

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


def _check_product(tag, got, ref, bar):
    err = np.abs(np.asarray(got).ravel() - np.asarray(ref).ravel())
    bar = np.asarray(bar).ravel()
    print("%s: max error / bar %.3e (max error %.3e of scale)" % (tag, (err / np.maximum(bar, 1e-300)).max(), err.max() / np.abs(ref).max()))
    assert np.all(np.isfinite(got)) and np.all(err <= bar)


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


# ------------------------------------------------------------------------------------------------ the product
@pytest.mark.parametrize("key", U.SMALL + [U.MID], ids=_name)
def test_geometric_apply_against_the_restatement(key):
    c = _context(key)
    en, pos = B.mesh_tables(key)
    assert np.array_equal(c.node_positions(), pos) and np.array_equal(c.elem_nodes(), en)      # the oracle's numbering is the library's own
    dim, deg = pos.shape[1], B.mesh_arrays(key)[2]
    x = _rand(dim * c.n_dof)
    sig = _sigma(key)
    c.set_prestress(sig)
    ref = B.geometric_stiffness(dim, deg, en, pos, sig) @ x
    bar = B.product_bound(dim, deg, en, pos, sig, x.reshape(-1, dim))
    got = c.geometric_apply(x)
    _check_product(_name(key), got, ref, bar)
    if key != U.MID:
        d = _Dev(c)                                      # device pointers: the field scanned by the flag kernel, the product in place on the device
        try:
            c.set_prestress(None)
            c._ck(c.lib.mfh_set_prestress(c.h, d.up(sig), len(sig), L.LOAD_ON_DEVICE))
            y = d.alloc(8 * x.size)
            c._ck(c.lib.mfh_geometric_apply(c.h, d.up(x), y, L.LOAD_ON_DEVICE))
            _check_product(_name(key) + " (device pointers)", d.down(y, x.shape), ref, bar)
        finally:
            d.free()
    c.close()


def test_geometric_apply_under_a_periodic_dof_map():
    """the unit cell with its interior perturbed, quadratic triangles: y = P^T Kg P x"""
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
    c.set_prestress(sig)
    x = _rand(2 * n_dof)
    ref = B.geometric_stiffness(2, 2, en, pos, sig, dof, n_dof) @ x
    bar = B.product_bound(2, 2, en, pos, sig, x.reshape(-1, 2), dof, n_dof)
    _check_product("periodic 2D-P2", c.geometric_apply(x), ref, bar)
    c.close()


@pytest.mark.parametrize("key", U.SMALL, ids=_name)
def test_unit_stress_is_the_contexts_laplacian(key):
    """sigma = I: Kg x equals the context's own MFH_OP_LAPLACIAN product applied to every component -- no restatement in the comparison; the bar is
    the product bound at sigma = I"""
    c = _context(key)
    en, pos = B.mesh_tables(key)
    dim, deg = key
    sig = B.uniform_field(len(en), dim, np.eye(dim))
    x = _rand(dim * c.n_dof).reshape(-1, dim)
    c.set_prestress(sig)
    got = c.geometric_apply(x)
    c.set_operator(M.OP_LAPLACIAN)
    c.assemble()
    ref = np.stack([c.apply_K(np.ascontiguousarray(x[:, a])) for a in range(dim)], axis=1)
    _check_product(_name(key), got, ref, B.product_bound(dim, deg, en, pos, sig, x))
    c.close()


@pytest.mark.parametrize("key,options", [((2, 1), ()), ((3, 1), ()), ((2, 2), ()), ((3, 2), ()), ((3, 2), (("matrix_storage", 0),)),
                                         ((3, 2), (("deterministic", 1),)), ((2, 2), (("deterministic", 1),))],
                         ids=["2D-P1-default", "3D-P1-default", "2D-P2-default", "3D-P2-default", "3D-P2-both-triangles", "3D-P2-deterministic",
                              "2D-P2-deterministic"])
def test_two_calls_give_the_same_bits(key, options):
    """Two calls on one context, and a call on a fresh context, return the same bits -- with default options, where the context stores the upper
    triangle and every call widens the pattern and reassembles Kg (the library always assembles Kg with the turn-taking flavour of the gather
    assembly), with both triangles stored (assembled once), and under option deterministic."""
    dim, deg = key
    x = _rand(dim * len(B.mesh_tables(key)[1]))
    c = _context(key, options=options)
    c.set_prestress(_sigma(key))
    y1, y2 = c.geometric_apply(x), c.geometric_apply(x)
    c.close()
    assert np.array_equal(y1, y2)
    f = _context(key, options=options)
    f.set_prestress(_sigma(key))
    assert np.array_equal(f.geometric_apply(x), y1)
    f.close()


# ------------------------------------------------------------------------------------------------ load factors
@functools.lru_cache(maxsize=None)
def _solve(key, precond):
    c = _context(key, precond)
    assert np.array_equal(c.node_positions(), B.mesh_tables(key)[1])
    c.fix_variables(B.clamp_vars(key))
    c.set_prestress(B.axial_compression(key))
    fac, X, info = c.buckling(NEV, rtol=RTOL, maxit=MAXIT)
    c.close()
    return fac, X, info


COLUMN_CASES = [(k, p) for k in B.COLUMNS for p in ("jacobi", "two-level", "multigrid")]


@pytest.mark.parametrize("key,precond", COLUMN_CASES, ids=_name)
def test_load_factors_against_dense_truth(key, precond):
    fac, X, info = _solve(key, precond)
    mu_ref, _, cond, _ = B.column_truth(key)
    mu_ref = mu_ref[:NEV]
    mu = -1.0 / fac
    bar = np.sqrt(cond) * RTOL * np.abs(mu_ref)
    err = np.abs(mu - mu_ref)
    print("%s %s: %d unknowns, %d iterations, block %d, restarts %d, precondUsed %d, factors %s, max err / bar %.3e, note '%s'" %
          (key, precond, len(B.free_vars(key)), info["iterations"], info["blockSize"], info["restarts"], info["precondUsed"], fac, (err / bar).max(), info["note"]))
    assert info["converged"] == 1 and info["maxResidual"] <= RTOL and info["nBuckling"] == NEV
    assert np.all(np.isfinite(fac)) and np.all(np.diff(fac) >= 0) and np.all(fac > 0)
    assert np.all(err <= bar)


@functools.lru_cache(maxsize=None)
def _device_K(key):
    c = _context(key)
    n = c.bs * c.n_dof
    c.assemble()
    i, j, v = c.export_upper_triplets()
    c.close()
    U_ = sp.coo_matrix((v, (i.astype(np.int64), j.astype(np.int64))), shape=(n, n)).tocsr()
    return sp.csr_matrix(U_ + sp.triu(U_, 1).T)


@pytest.mark.parametrize("key,precond", COLUMN_CASES, ids=_name)
def test_residuals_orthonormality_clamp_and_sign(key, precond):
    fac, X, info = _solve(key, precond)
    mu = -1.0 / fac
    f = B.free_vars(key)
    K = _device_K(key)
    Kg = B.Kg_of(key, B.axial_compression(key))
    res = B.host_residuals(K[f][:, f], Kg[f][:, f], mu, X[:, f])
    Ko = B.stiffness(key)
    n = X.shape[1]
    defect = np.abs(X @ (Ko @ X.T) - np.eye(len(X))).max()
    defect_ref = B.column_truth(key)[3]
    print("%s %s: residuals recomputed %s reported %s; defect %.3e, eigh's %.3e, n eps %.3e" % (key, precond, res, info["residuals"], defect, defect_ref, n * EPS))
    assert np.all(res <= 2 * RTOL)
    assert defect <= max(10 * defect_ref, n * EPS)
    assert np.all(X[:, B.clamp_vars(key)] == 0.0)
    assert U.sign_rule_holds(X)


# ------------------------------------------------------------------------------------------------ the chain load -> u -> prestress -> factors
def test_simulator_chain_under_a_top_traction():
    """Simulator.buckling on the linear column, clamped at the bottom nodes, pushed down by a traction on its top face. The reference takes the DEVICE's u,
    rebuilds sigma with the oracle's average stress and Kg in numpy, and runs eigh: the eigenvalue bar. Scaling the load by 3 divides the factors by 3
    (both sides carry the bar)."""
    from oracle import meshfem_oracle as O
    from meshfem_amd.linear_elasticity import Simulator
    key = "col3d-P1"
    V, T, deg, _ = B.mesh_arrays(key)
    sim = Simulator(T, V, deg)
    sim.rtol = 1e-11
    sim.setIsotropicMaterial(U.E_MOD, U.NU)
    fixed = B.clamp_vars(key)
    nodes = np.unique(fixed // 3)
    sim.applyDirichletNodes(nodes, np.zeros((len(nodes), 3)))
    sim.applyNeumannBox([-0.01, -0.01, 0.985], [1.01, 1.01, 1.01], [0, 0, -1.0], relative=True)
    load = sim.neumannLoad()
    assert abs(load[:, 2].sum() + 6.0) <= 0.2                                     # the top face (area about 3 x 2) carries the traction
    fac, modes, u = sim.buckling(NEV, maxit=MAXIT)
    info = sim.buckling_info
    assert info["converged"] == 1 and modes.shape == (NEV, sim.numNodes(), 3) and u.shape == (sim.numNodes(), 3)
    osim = O.Simulator(T, V, deg, mesh=B.fem_mesh(key))
    osim.set_material_constant(O.ElasticityTensor.isotropic(3, U.E_MOD, U.NU))
    sigma = osim.averageStressField(u)
    en, pos = B.mesh_tables(key)
    f = B.free_vars(key)
    Kf = B.stiffness(key)[f][:, f].toarray()
    Gf = B.geometric_stiffness(3, deg, en, pos, sigma)[f][:, f].toarray()
    mu_ref = scipy.linalg.eigh(Gf, Kf, eigvals_only=True)[:NEV]
    cond = B.column_truth(key)[2]
    bar = np.sqrt(cond) * RTOL * np.abs(mu_ref)
    err = np.abs(-1.0 / fac - mu_ref)
    print("chain: factors %s (uniform compression of the same resultant: %s), %d iterations, max err / bar %.3e" %
          (fac, B.factors_of(B.column_truth(key)[0][:NEV]), info["iterations"], (err / bar).max()))
    assert np.all(err <= bar)
    fac3, _, u3 = sim.buckling(NEV, load=3.0 * load, maxit=MAXIT)
    print("chain: 3 x factors(3 x load) / factors(load) - 1 = %s" % (3.0 * fac3 / fac - 1))
    assert np.all(np.abs(3.0 * fac3 / fac - 1) <= 2 * np.sqrt(cond) * RTOL)
    sim.ctx.close()


# ------------------------------------------------------------------------------------------------ state
@pytest.mark.parametrize("key", [(2, 2), (3, 1)], ids=_name)
def test_state_of_the_field(key):
    dim, deg = key
    en, pos = B.mesh_tables(key)
    a, b = _sigma(key, 3), _sigma(key, 4)
    x = _rand(dim * len(pos))
    c = _context(key)
    c.fix_variables(U.clamp_vars(key))

    def check(sig, en_, pos_):
        _check_product(_name(key), c.geometric_apply(x), B.geometric_stiffness(dim, deg, en_, pos_, sig) @ x,
                       B.product_bound(dim, deg, en_, pos_, sig, x.reshape(-1, dim)))
    c.set_prestress(a)
    check(a, en, pos)
    c.set_prestress(b)                                    # a changed field reassembles
    check(b, en, pos)
    assert np.abs(c.geometric_apply(x) - B.geometric_stiffness(dim, deg, en, pos, a) @ x).max() > 1e-3
    V, T, _, _ = U.mesh_arrays(key)                        # a vertex update keeps the field and invalidates the buffer
    c.mesh_update_vertices(np.ascontiguousarray(V * 1.25))
    check(b, c.elem_nodes(), c.node_positions())
    c.set_prestress(None)                                 # NULL clears: nothing to multiply by, nothing to buckle under
    y = np.empty_like(x)
    assert c.lib.mfh_geometric_apply(c.h, ptr(x), ptr(y), 0) == L.ERR_STATE
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.buckling(1, rtol=RTOL, maxit=MAXIT)
    assert ei.value.code == L.ERR_STATE
    c.set_prestress(b)                                    # a new mesh clears the field
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    assert c.lib.mfh_geometric_apply(c.h, ptr(x), ptr(y), 0) == L.ERR_STATE
    c.set_prestress(a)
    check(a, en, pos)
    c.close()


def test_prestress_from_displacement_is_the_average_stress():
    """the field written on the device is what average_stress returns: the products agree to the last bit (option deterministic: every new field reassembles)"""
    key = (3, 2)
    c = _context(key, options=(("matrix_storage", 0), ("deterministic", 1)))
    u = _rand(c.n_node * 3).reshape(-1, 3)
    x = _rand(3 * c.n_dof)
    c.prestress_from_displacement(u)
    y1 = c.geometric_apply(x)
    c.set_prestress(c.average_stress(u))
    assert np.array_equal(c.geometric_apply(x), y1)
    d = _Dev(c)
    try:
        c._ck(c.lib.mfh_prestress_from_displacement(c.h, d.up(u), L.LOAD_ON_DEVICE))
        assert np.array_equal(c.geometric_apply(x), y1)
    finally:
        d.free()
    c.close()


# ------------------------------------------------------------------------------------------------ nothing existing moves
def _probe(c):
    n = c.bs * c.n_dof
    rng = np.random.default_rng(5)
    f, x = rng.standard_normal(n), rng.standard_normal(n)
    u = c.solve(f, rtol=1e-9)
    return u, c.apply_K(x), c.export_upper_triplets(), c.modes(3, rtol=RTOL)[:2]


@pytest.mark.parametrize("storage", [-1, 0], ids=["default-storage", "both-triangles"])
def test_nothing_existing_moves(storage):
    """A context that has run mfh_buckling solves, applies K, exports and computes its vibrational modes like a fresh one, bit for bit -- also the
    default quadratic context, whose pattern the call widened for its own duration (both contexts with option deterministic 1, as in
    tests/test_gpu_modes.py)."""
    key = (3, 2)
    opts = (("deterministic", 1), ("matrix_storage", storage))
    fixed = U.clamp_vars(key)
    en, _ = B.mesh_tables(key)
    S = np.zeros((3, 3))
    S[0, 0] = -1.0                                        # compression along x, the axis the clamp is normal to
    a = _context(key, "multigrid", opts)
    a.fix_variables(fixed)
    a.set_prestress(B.uniform_field(len(en), 3, S))
    fac, X, info = a.buckling(3, rtol=RTOL, maxit=MAXIT)
    assert info["converged"] == 1 and ("both triangles" in info["note"]) == (storage == -1)
    got = _probe(a)
    b = _context(key, "multigrid", opts)
    b.fix_variables(fixed)
    want = _probe(b)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for g, w_ in zip(got[2], want[2]):
        assert np.array_equal(g, w_)
    assert np.array_equal(got[3][0], want[3][0]) and np.array_equal(got[3][1], want[3][1])
    fac2, X2, _ = a.buckling(3, rtol=RTOL, maxit=MAXIT)  # and two calls give the same bits
    assert np.array_equal(fac, fac2) and np.array_equal(X, X2)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ tension, edge cases, refusals
def test_tension_does_not_buckle():
    key = "strip-P1"
    c = _context(key)
    c.fix_variables(B.clamp_vars(key))
    c.set_prestress(B.axial_compression(key, -1.0))
    st = None
    try:
        c.buckling(NEV, rtol=RTOL, maxit=30)
    except M.MeshFEMHipError as e:
        st = e.code
    fac, X, info = c.last_buckling
    print("tension: status %s, %d iterations, factors %s" % (st, info["iterations"], fac))
    assert st in (None, L.ERR_NOT_CONVERGED)
    assert info["nBuckling"] == 0 and np.all(np.isposinf(fac)) and np.all(np.isfinite(X))
    c.close()


def test_maxit_two():
    key = "col3d-P2"
    c = _context(key)
    c.fix_variables(B.clamp_vars(key))
    c.set_prestress(B.axial_compression(key))
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.buckling(NEV, rtol=RTOL, maxit=2)
    assert ei.value.code == L.ERR_NOT_CONVERGED
    fac, X, info = c.last_buckling
    assert info["iterations"] == 2 and info["converged"] == 0
    assert np.all(fac > 0) and np.all(np.isfinite(fac)) and np.all(np.isfinite(X)) and np.all(np.diff(fac) >= 0)
    u = c.solve(np.ones(c.bs * c.n_dof), rtol=1e-8)
    assert c.last_info["converged"] == 1 and np.all(np.isfinite(u))
    c.close()


def test_refusals():
    key = (2, 1)
    c = _context(key)
    c.fix_variables(U.clamp_vars(key))
    n_elem, fl = c.n_elem, 3
    good = np.array(_sigma(key))
    c.set_prestress(good)
    x = _rand(c.dim * c.n_dof)
    before = c.geometric_apply(x)
    lib = c.lib
    n = c.dim * c.n_dof
    fac, X, res = np.zeros(21), np.zeros((21, n)), np.zeros(21)
    info = L.BucklingInfo()

    def refused(status, code=L.ERR_INVALID):
        """the call was refused with `code` and the field in force is untouched"""
        assert status == code
        assert np.abs(c.geometric_apply(x) - before).max() <= 1e-14 * np.abs(before).max()
    d = _Dev(c)
    try:
        for v in (np.nan, np.inf, -np.inf):
            bad = np.array(good)
            bad[n_elem // 2, 1] = v
            refused(lib.mfh_set_prestress(c.h, ptr(bad), n_elem, 0))
            refused(lib.mfh_set_prestress(c.h, d.up(bad), n_elem, L.LOAD_ON_DEVICE))
        for cnt in (n_elem - 1, n_elem + 1, 0, n_elem * fl):
            refused(lib.mfh_set_prestress(c.h, ptr(good), cnt, 0))
            refused(lib.mfh_set_prestress(c.h, d.up(good), cnt, L.LOAD_ON_DEVICE))
        refused(lib.mfh_set_prestress(c.h, ptr(good), n_elem, 4))
        refused(lib.mfh_prestress_from_displacement(c.h, ptr(np.zeros(n)), 4))
        refused(lib.mfh_prestress_from_displacement(c.h, None, 0))
        y = np.empty_like(before)
        refused(lib.mfh_geometric_apply(c.h, None, ptr(y), 0))
        refused(lib.mfh_geometric_apply(c.h, ptr(x), ptr(y), 1))
        n_free = n - len(U.clamp_vars(key))
        for nev in (0, 21, -1):
            refused(lib.mfh_buckling(c.h, nev, 0, RTOL, 100, ptr(fac), ptr(X), ptr(res), C.byref(info)))
        refused(lib.mfh_buckling(c.h, 1, 1, RTOL, 100, ptr(fac), ptr(X), ptr(res), C.byref(info)))
        assert n_free > 20
        with pytest.raises(ValueError):
            c.geometric_apply(x[:-1])
        with pytest.raises(ValueError):
            c.set_prestress(good[:, :2])
        # a clamp that leaves rigid motions free
        c.clear_fixed()
        c.fix_variables([0, 1])
        refused(lib.mfh_buckling(c.h, 1, 0, RTOL, 100, ptr(fac), ptr(X), ptr(res), C.byref(info)), L.ERR_UNSUPPORTED)
        c.clear_fixed()
        refused(lib.mfh_buckling(c.h, 1, 0, RTOL, 100, ptr(fac), ptr(X), ptr(res), C.byref(info)), L.ERR_UNSUPPORTED)
        # more modes than the pencil has: all but two variables fixed
        c.fix_variables(np.arange(n - 2))
        refused(lib.mfh_buckling(c.h, 3, 0, RTOL, 100, ptr(fac), ptr(X), ptr(res), C.byref(info)))
        c.clear_fixed()
        c.fix_variables(U.clamp_vars(key))
        # an operator other than elasticity; the forced-degree-1 view
        c.set_operator(M.OP_LAPLACIAN)
        assert lib.mfh_buckling(c.h, 1, 0, RTOL, 100, ptr(fac), ptr(X), ptr(res), C.byref(info)) == L.ERR_UNSUPPORTED
        assert lib.mfh_geometric_apply(c.h, ptr(x), ptr(y), 0) == L.ERR_UNSUPPORTED
        assert lib.mfh_prestress_from_displacement(c.h, ptr(np.zeros(n)), 0) == L.ERR_UNSUPPORTED
        c.set_operator(M.OP_ELASTICITY)
        c.fix_variables(U.clamp_vars(key))
        assert np.abs(c.geometric_apply(x) - before).max() <= 1e-14 * np.abs(before).max()
    finally:
        d.free()
    c.close()
    q = _context((2, 2))
    q.set_prestress(_sigma((2, 2)))
    q.set_operator(M.OP_LAPLACIAN)
    q.set_operator_degree(1)
    xq = np.zeros(2 * q._n_dof_full)
    assert q.lib.mfh_buckling(q.h, 1, 0, RTOL, 100, ptr(fac), ptr(np.zeros((1, xq.size))), ptr(res), C.byref(info)) == L.ERR_UNSUPPORTED
    assert q.lib.mfh_geometric_apply(q.h, ptr(xq), ptr(xq.copy()), 0) == L.ERR_UNSUPPORTED
    q.close()
    # MFH_ERR_STATE: no mesh; a matrix from mfh_matrix_set_upper_triplets; a host-only context; no prestress
    one = np.ones(6)
    e = M.Context(0)
    assert e.lib.mfh_set_prestress(e.h, ptr(one), 2, 0) == L.ERR_STATE
    assert e.lib.mfh_prestress_from_displacement(e.h, ptr(one), 0) == L.ERR_STATE
    assert e.lib.mfh_geometric_apply(e.h, ptr(one), ptr(one.copy()), 0) == L.ERR_STATE
    assert e.lib.mfh_buckling(e.h, 1, 0, RTOL, 100, ptr(fac), ptr(X), ptr(res), C.byref(info)) == L.ERR_STATE
    e.matrix_set_upper_triplets(3, [0, 1, 2], [0, 1, 2], [1.0, 2.0, 3.0])
    assert e.lib.mfh_set_prestress(e.h, ptr(one), 2, 0) == L.ERR_STATE
    assert e.lib.mfh_prestress_from_displacement(e.h, ptr(one), 0) == L.ERR_STATE
    assert e.lib.mfh_geometric_apply(e.h, ptr(one), ptr(one.copy()), 0) == L.ERR_STATE
    assert e.lib.mfh_buckling(e.h, 1, 0, RTOL, 100, ptr(fac), ptr(X), ptr(res), C.byref(info)) == L.ERR_STATE
    e.close()
    V, T, deg, _ = U.mesh_arrays(key)
    h = M.Context(-1)
    h.mesh_build(T, V, deg)
    assert h.lib.mfh_set_prestress(h.h, ptr(good), n_elem, 0) == L.ERR_STATE
    assert h.lib.mfh_prestress_from_displacement(h.h, ptr(np.zeros(n)), 0) == L.ERR_STATE
    assert h.lib.mfh_geometric_apply(h.h, ptr(x), ptr(x.copy()), 0) == L.ERR_STATE
    assert h.lib.mfh_buckling(h.h, 1, 0, RTOL, 100, ptr(fac), ptr(X), ptr(res), C.byref(info)) == L.ERR_STATE
    h.close()
    g = _context(key)
    g.fix_variables(U.clamp_vars(key))
    assert g.lib.mfh_buckling(g.h, 1, 0, RTOL, 100, ptr(fac), ptr(X), ptr(res), C.byref(info)) == L.ERR_STATE
    assert g.lib.mfh_geometric_apply(g.h, ptr(x), ptr(x.copy()), 0) == L.ERR_STATE
    g.close()
    # MFH_ERR_UNSUPPORTED: a row-partitioned context
    p = M.Context(0)
    p.mesh_set(2, 1, T, V, n_owned=len(V) - 3)
    p.material_isotropic(U.E_MOD, U.NU)
    assert p.lib.mfh_set_prestress(p.h, ptr(good), n_elem, 0) == L.ERR_UNSUPPORTED
    assert p.lib.mfh_set_prestress(p.h, None, 0, 0) == L.ERR_UNSUPPORTED
    assert p.lib.mfh_prestress_from_displacement(p.h, ptr(np.zeros(2 * len(V))), 0) == L.ERR_UNSUPPORTED
    assert p.lib.mfh_geometric_apply(p.h, ptr(np.ones(2 * len(V))), ptr(np.ones(2 * len(V))), 0) == L.ERR_UNSUPPORTED
    assert p.lib.mfh_buckling(p.h, 1, 0, RTOL, 100, ptr(fac), ptr(X), ptr(res), C.byref(info)) == L.ERR_UNSUPPORTED
    p.close()
