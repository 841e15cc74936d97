"""mfh_modes on the device against scipy: the smallest eigenpairs of K x = lambda M x, clamped and free-free, on the small meshes of
tests/test_gpu_differential_operators.py (3 x 2 x 2 tets, 4 x 3 triangles, perturbed, P1 and P2), on one mid-size mesh whose kernels span many
workgroups (8 x 7 x 6 quadratic tets, 37 905 unknowns) and on an unperturbed square bar with double bending modes. rtol = 1e-6 throughout.
Bars (tests/modes_util.py computes what they need):
  eigenvalues      |lambda~ - lambda| <= sqrt(cond2(M_ff)) rtol lambda: the first-order residual bound, ||r||_M^-1 / ||M x||_M^-1 <= sqrt(cond M) residual
  residuals        recomputed on the host from the matrices a second context exports: <= 2 rtol, and within a factor 2 of the reported ones
  orthonormality   ||X M X^T - I||_max <= max(10 x the defect of scipy's own eigenvectors on the case, n eps)
Every solve is made once (functools.lru_cache) and shared by the tests that look at it."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import meshfem_amd as M
from meshfem_amd import _lib

import modes_util as U

pytestmark = pytest.mark.gpu

RTOL = 1e-6
EPS = U.EPS
PRECONDS = {"jacobi": M.PRECOND_BLOCK_JACOBI, "two-level": M.PRECOND_TWO_LEVEL, "multigrid": M.PRECOND_MULTIGRID}
MESHES = U.SMALL + [U.MID]


def _is3d(key):
    return key == U.MID or key == U.BAR or key[0] == 3


def _name(key):
    return key if isinstance(key, str) else "%dD-P%d" % key


def _context(key, precond="jacobi", options=()):
    V, T, deg, _ = U.mesh_arrays(key)
    c = M.Context(0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    c.set_preconditioner(PRECONDS[precond])
    return c


@functools.lru_cache(maxsize=None)
def _clamped(key, precond, nev):
    c = _context(key, precond)
    assert np.array_equal(c.node_positions(), U.fem_mesh(key).node_pos)          # the oracle's node numbering is the library's own
    c.fix_variables(U.clamp_vars(key, 2 if key == U.BAR else 0))
    lam, X, info = c.modes(nev, rtol=RTOL, maxit=3000)
    c.close()
    return lam, X, info


@functools.lru_cache(maxsize=None)
def _free(key, precond, nev=4):
    c = _context(key, precond)
    lam, X, info = c.modes(nev, free=True, rtol=RTOL, maxit=3000)
    c.close()
    return lam, X, info


CLAMPED_CASES = [(k, "jacobi") for k in MESHES] + [(k, p) for k in MESHES if _is3d(k) for p in ("two-level", "multigrid")]


@pytest.mark.parametrize("nev", [1, 4, 7])
@pytest.mark.parametrize("key,precond", CLAMPED_CASES, ids=_name)
def test_clamped_eigenvalues(key, precond, nev):
    """All nodes of the face x = min fixed. The sorted smallest eigenvalues of the free-free block of (K, M): a skipped mode shows as a shifted list."""
    lam, X, info = _clamped(key, precond, nev)
    ref, _, cond, _ = U.clamped_truth(key)
    bar = np.sqrt(cond) * RTOL * ref[:nev]
    err = np.abs(lam - ref[:nev])
    print("%s %s nev %d: %d iterations, block %d, restarts %d, max err / bar %.3e, note '%s'" %
          (_name(key), precond, nev, info["iterations"], info["blockSize"], info["restarts"], (err / bar).max(), info["note"]))
    assert info["converged"] == 1 and info["maxResidual"] <= RTOL
    assert np.all(np.diff(lam) >= 0)
    assert np.all(err <= bar)
    if key == U.MID:
        assert info["precondUsed"] == PRECONDS[precond]


@functools.lru_cache(maxsize=None)
def _device_pencil(key):
    """(K, M) as the DEVICE holds them: a second context's upper triplets under each operator (then only rounding differs from what mfh_modes used)."""
    c = _context(key)
    n = c.bs * c.n_dof
    c.assemble()
    i, j, v = c.export_upper_triplets()
    U_ = sp.coo_matrix((v, (i.astype(np.int64), j.astype(np.int64))), shape=(n, n)).tocsr()
    K = U_ + sp.triu(U_, 1).T
    c.set_operator(M.OP_MASS_VECTOR)
    c.assemble()
    i, j, v = c.export_upper_triplets()
    U_ = sp.coo_matrix((v, (i.astype(np.int64), j.astype(np.int64))), shape=(n, n)).tocsr()
    Mm = U_ + sp.triu(U_, 1).T
    c.close()
    return sp.csr_matrix(K), sp.csr_matrix(Mm)


RESIDUAL_CASES = [((2, 1), "jacobi"), ((2, 2), "jacobi"), ((3, 1), "two-level"), ((3, 2), "multigrid"), (U.MID, "multigrid")]


@pytest.mark.parametrize("key,precond", RESIDUAL_CASES, ids=_name)
def test_residuals_recomputed_on_the_host(key, precond):
    lam, X, info = _clamped(key, precond, 4)
    K, Mm = _device_pencil(key)
    f = U.free_vars(key, U.clamp_vars(key))
    res = U.host_residuals(K[f][:, f], Mm[f][:, f], lam, X[:, f])
    print("%s: recomputed %s reported %s" % (_name(key), res, info["residuals"]))
    assert np.all(res <= 2 * RTOL)
    assert np.all(info["residuals"] <= 2 * res) and np.all(res <= 2 * info["residuals"])


@pytest.mark.parametrize("key,precond", RESIDUAL_CASES, ids=_name)
def test_orthonormality_clamp_and_sign(key, precond):
    lam, X, info = _clamped(key, precond, 4)
    _, Mm = U.pencil(key)
    _, _, _, defect_ref = U.clamped_truth(key)
    n = X.shape[1]
    defect = np.abs(X @ (Mm @ X.T) - np.eye(len(X))).max()
    print("%s: defect %.3e, scipy's %.3e, n eps %.3e" % (_name(key), defect, defect_ref, n * EPS))
    assert defect <= max(10 * defect_ref, n * EPS)
    fixed = U.clamp_vars(key)
    assert np.all(X[:, fixed] == 0.0)
    assert U.sign_rule_holds(X)


FREE_CASES = [(k, "jacobi") for k in U.SMALL] + [((3, 1), "two-level"), ((3, 2), "multigrid"), (U.MID, "multigrid")]


@pytest.mark.parametrize("key,precond", FREE_CASES, ids=_name)
def test_free_free(key, precond):
    """The smallest NON-ZERO eigenvalues: the dense truth after dropping its 3 / 6 zeros (mid mesh: eigsh about a small negative shift);
    the modes are M-orthogonal to the rigid-body modes to the orthonormality bar."""
    nev = 4
    lam, X, info = _free(key, precond)
    K, Mm = U.pencil(key)
    m = U.fem_mesh(key)
    nz = 6 if m.N == 3 else 3
    ref, _, cond, defect_ref = U.free_truth(key)
    ref = ref[nz:nz + nev]
    bar = np.sqrt(cond) * RTOL * ref
    err = np.abs(lam - ref)
    print("%s %s: %d iterations, max err / bar %.3e, note '%s'" % (_name(key), precond, info["iterations"], (err / bar).max(), info["note"]))
    assert info["converged"] == 1
    assert np.all(err <= bar)
    n = X.shape[1]
    tol = max(10 * defect_ref, n * EPS)
    assert np.abs(X @ (Mm @ X.T) - np.eye(nev)).max() <= tol
    Z = U.m_orthonormalise(U.rigid_modes(m.node_pos), Mm)
    assert np.abs(Z.T @ (Mm @ X.T)).max() <= tol
    assert U.sign_rule_holds(X)
    if precond == "two-level":
        assert info["precondUsed"] == M.PRECOND_BLOCK_JACOBI and "block-Jacobi" in info["note"]


def test_free_free_refusals():
    c = _context((3, 1))
    c.fix_variables([0])
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes(2, free=True)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    c.clear_fixed()
    # a clamp that leaves rigid motions free goes through the posedness message
    c.fix_variables([0, 1, 2])
    with pytest.raises(M.MeshFEMHipError, match="rigid motions free") as ei:
        c.modes(2)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    c.close()
    c = _context(U.BAR)
    assert c.apply_periodic_conditions() < c.n_node
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes(2, free=True)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    c.close()


def test_multiplicity_square_bar():
    """The unperturbed 2 x 2 x 6 linear bar clamped at z = min: bending about x and about y come in (near-)equal pairs; nev = 4 must return both
    members of each pair. Values only: inside a pair the vectors are not unique."""
    key = U.BAR
    lam, X, info = _clamped(key, "jacobi", 4)
    K, Mm = U.pencil(key)
    f = U.free_vars(key, U.clamp_vars(key, 2))
    import scipy.linalg
    ref = scipy.linalg.eigh(K[f][:, f].toarray(), Mm[f][:, f].toarray(), eigvals_only=True)
    cond = np.linalg.cond(Mm[f][:, f].toarray())
    print("bar: lambda %s, truth %s" % (lam, ref[:6]))
    assert info["converged"] == 1
    assert np.all(np.abs(lam - ref[:4]) <= np.sqrt(cond) * RTOL * ref[:4])


def _probe(c, key):
    """What test_nothing_existing_moves compares: a solve, K x, the exported triplets."""
    n = c.bs * c.n_dof
    rng = np.random.default_rng(5)
    f, x = rng.standard_normal(n), rng.standard_normal(n)
    u = c.solve(f, rtol=1e-9)
    return u, c.apply_K(x), c.export_upper_triplets()


@pytest.mark.parametrize("storage", [-1, 0], ids=["default-storage", "both-triangles"])
def test_nothing_existing_moves(storage):
    """A context that has run mfh_modes solves, applies K and exports like a fresh one, bit for bit -- also the default quadratic context, whose
    pattern the call widened to both triangles for its own duration. Both contexts run with option deterministic 1: the default kernels add in
    arrival order, and two FRESH contexts already differ in their last bits (tests/test_gpu_deterministic.py)."""
    key = (3, 2)
    opts = (("deterministic", 1), ("matrix_storage", storage))
    fixed = U.clamp_vars(key)
    a = _context(key, "multigrid", opts)
    a.fix_variables(fixed)
    lam, X, info = a.modes(3, rtol=RTOL)
    assert ("both triangles" in info["note"]) == (storage == -1)
    got = _probe(a, key)
    b = _context(key, "multigrid", opts)
    b.fix_variables(fixed)
    want = _probe(b, key)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for g, w_ in zip(got[2], want[2]):
        assert np.array_equal(g, w_)
    # the operator switch is untouched by the resident mass buffer: the same export as on the fresh context ...
    a.set_operator(M.OP_MASS_VECTOR); b.set_operator(M.OP_MASS_VECTOR)
    a.assemble(); b.assemble()
    ma, mb = a.export_upper_triplets(), b.export_upper_triplets()
    for g, w_ in zip(ma, mb):
        assert np.array_equal(g, w_)
    # ... and it holds the matrix the modes are orthonormal in (density 1: the resident buffer times 1.0)
    n = X.shape[1]
    Um = sp.coo_matrix((ma[2], (ma[0].astype(np.int64), ma[1].astype(np.int64))), shape=(n, n)).tocsr()
    Mm = Um + sp.triu(Um, 1).T
    assert np.abs(X @ (Mm @ X.T) - np.eye(len(X))).max() <= max(10 * U.clamped_truth(key)[3], n * EPS)
    # two calls give the same bits
    a.set_operator(M.OP_ELASTICITY); a.fix_variables(fixed)
    l1, X1, _ = a.modes(3, rtol=RTOL)
    l2, X2, _ = a.modes(3, rtol=RTOL)
    assert np.array_equal(l1, l2) and np.array_equal(X1, X2)
    assert np.array_equal(l1, lam) and np.array_equal(X1, X)
    a.close(); b.close()


def test_maxit_two():
    key = (3, 2)
    c = _context(key, "jacobi")
    c.fix_variables(U.clamp_vars(key))
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes(4, rtol=RTOL, maxit=2)
    assert ei.value.code == _lib.ERR_NOT_CONVERGED
    lam, X, info = c.last_modes
    assert info["iterations"] == 2 and info["converged"] == 0
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(X)) and np.all(lam > 0)
    n = c.bs * c.n_dof
    u = c.solve(np.ones(n), rtol=1e-8)
    assert c.last_info["converged"] == 1 and np.all(np.isfinite(u))
    c.close()


def test_simulator_layer_on_the_golden_cantilever():
    """Simulator.vibrational_modes on tests/golden/cantilever (20 x 4 x 4 grid, the Dirichlet box of cantilever.bc, the material and density of
    B9Creator.material): frequencies = sqrt(lambda) / 2 pi of the C call on a context set up by hand, modes as [nev, nNode, 3]."""
    import json
    from meshfem_amd import grid
    from meshfem_amd.linear_elasticity import Simulator
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cantilever")
    bc = json.load(open(os.path.join(gold, "cantilever.bc")))
    mat = json.load(open(os.path.join(gold, "B9Creator.material")))
    box = [r for r in bc["regions"] if r["type"] == "dirichlet"][0]["box%"]
    V, T = grid.grid_tet_mesh(20, 4, 4)
    sim = Simulator(T, V, 2)
    sim.ctx.set_option("deterministic", 1)
    sim.ctx.set_preconditioner(M.PRECOND_MULTIGRID)
    sim.setIsotropicMaterial(mat["young"], mat["poisson"])
    sim.applyDirichletBox(box["minCorner"], box["maxCorner"], [0, 0, 0], relative=True)
    freq, modes = sim.vibrational_modes(3, density=mat["density"])
    assert sim.modes_info["converged"] == 1 and modes.shape == (3, sim.numNodes(), 3)
    c = M.Context(0)
    c.set_option("deterministic", 1)
    c.mesh_build(T, V, 2)
    c.material_isotropic(mat["young"], mat["poisson"])
    c.set_preconditioner(M.PRECOND_MULTIGRID)
    c.bc_dirichlet_box(box["minCorner"], box["maxCorner"], [0, 0, 0], relative=True)
    v, _ = c.bc_dirichlet_vars()
    c.fix_variables(v)
    lam, X, _ = c.modes(3, density=mat["density"], rtol=1e-6, maxit=500)
    assert np.array_equal(freq, np.sqrt(lam) / (2 * np.pi))
    assert np.array_equal(modes.reshape(3, -1), X)
    assert freq[0] > 0 and np.all(np.diff(freq) >= 0)
    c.close()
