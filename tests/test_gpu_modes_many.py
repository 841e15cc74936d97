"""mfh_modes_many on the device against dense references: more modes than one block of the loop holds, computed batch by batch in the
M-orthogonal complement of everything found or handed in. Fixtures of tests/modes_util.py, rtol = 1e-6 throughout. Bars, on every case:
  eigenvalues      |lambda~ - lambda| <= sqrt(cond2(M_ff)) rtol lambda (the bar of tests/test_gpu_modes.py: a theorem for the nearest eigenvalue once the
                   full residual is <= rtol). The smallest relative gap among the first 60 eigenvalues of the fixtures is 1.7e-3, the bars are
                   <= 9e-6: every value is compared one to one, a skipped mode shows as a shifted list.
  residuals        recomputed on the host from the matrices a second context exports: <= 2 rtol. Where the locked set is arbitrary (no eigenvectors)
                   an eigenvector x of the restricted pencil has K x - lambda M x = M Q mu, not 0: there the residual is that of the restricted
                   pencil, r - M Q (Q^T r) with Q M-orthonormal
  orthonormality   ||X M X^T - I||_max over the whole returned set and ||Q M X^T||_max <= max(10 x the defect of scipy's own vectors, n eps)
  the clamp and the sign rule
Every solve is made once (functools.lru_cache) and shared by the tests that look at it."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import meshfem_amd as M
from meshfem_amd import _lib

import modes_util as U
import modes_many_util as MU

pytestmark = pytest.mark.gpu

RTOL = 1e-6
EPS = U.EPS
PRECONDS = {"jacobi": M.PRECOND_BLOCK_JACOBI, "two-level": M.PRECOND_TWO_LEVEL, "multigrid": M.PRECOND_MULTIGRID}


def _name(key):
    return key if isinstance(key, str) else "%dD-P%d" % key


def _context(key, precond="jacobi", options=(), clamp=True):
    V, T, deg, _ = U.mesh_arrays(key)
    c = M.Context(0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_build(T, V, deg)
    c.material_isotropic(U.E_MOD, U.NU)
    c.set_preconditioner(PRECONDS[precond])
    if clamp:
        c.fix_variables(U.clamp_vars(key, MU.clamp_axis(key)))
    return c


@functools.lru_cache(maxsize=None)
def _device_pencil(key):
    """(K, M) as the DEVICE holds them: a second context's upper triplets under each operator."""
    c = _context(key, clamp=False)
    n = c.bs * c.n_dof
    out = []
    for op in (M.OP_ELASTICITY, M.OP_MASS_VECTOR):
        c.set_operator(op)
        c.assemble()
        i, j, v = c.export_upper_triplets()
        U_ = sp.coo_matrix((v, (i.astype(np.int64), j.astype(np.int64))), shape=(n, n)).tocsr()
        out.append(sp.csr_matrix(U_ + sp.triu(U_, 1).T))
    c.close()
    return tuple(out)


def _check_set(key, lam, X, info, ref, cond, defect_ref, Q=None, free=False, restricted=False):
    """The bars of the module docstring on one returned set; ref: the true eigenvalues at the positions of lam. Q: [nq, n] M-orthonormal rows;
    restricted: the residuals are those of the pencil restricted to the complement of Q."""
    nev = len(lam)
    bar = MU.eig_bar(cond, RTOL, ref)
    err = np.abs(lam - ref)
    K, Mm = _device_pencil(key)
    n = X.shape[1]
    f = np.arange(n) if free else U.free_vars(key, U.clamp_vars(key, MU.clamp_axis(key)))
    Kf, Mf = K[f][:, f], Mm[f][:, f]
    if restricted:
        R = Kf @ X[:, f].T - (Mf @ X[:, f].T) * lam[None, :]
        MQ = Mf @ Q[:, f].T
        R = R - MQ @ (Q[:, f] @ R)
        res = np.linalg.norm(R, axis=0) / (lam * np.linalg.norm(Mf @ X[:, f].T, axis=0))
    else:
        res = U.host_residuals(Kf, Mf, lam, X[:, f])
    tol = max(10 * defect_ref, n * EPS)
    defect = np.abs(X @ (Mm @ X.T) - np.eye(nev)).max()
    qdefect = 0.0 if Q is None else np.abs(Q @ (Mm @ X.T)).max()
    print("%s: %d modes in %d batches, %d iterations, max err / bar %.3e, max residual / rtol host %.3e device %.3e, defect %.3e against Q %.3e (bar %.3e), "
          "lock defect %.3e, note '%s'" % (_name(key), nev, info["batches"], info["iterations"], (err / bar).max(), res.max() / RTOL,
                                           info["maxResidual"] / RTOL, defect, qdefect, tol, info["maxLockDefect"], info["note"]))
    assert info["converged"] == 1 and info["nFound"] == nev and info["maxResidual"] <= RTOL
    assert np.all(np.diff(lam) >= 0)
    assert np.all(err <= bar)
    assert np.all(res <= 2 * RTOL)
    assert np.all(info["residuals"] <= 2 * res + 1e-3 * RTOL) and np.all(res <= 2 * info["residuals"] + 1e-3 * RTOL)
    assert defect <= tol and qdefect <= tol
    if not free:
        assert np.all(X[:, U.clamp_vars(key, MU.clamp_axis(key))] == 0.0)
    assert U.sign_rule_holds(X)


# ---------------------------------------------------------------- arbitrary Q
@pytest.mark.parametrize("key", [(3, 1), (2, 2)], ids=_name)
def test_arbitrary_locked_set(key):
    """Q = 7 random vectors (no eigenvectors), nev = 6: the restricted dense truth."""
    Kf, Mf, f, cond = MU.dense_clamped(key)
    n = U.pencil(key)[0].shape[0]
    Qf = MU.random_set(len(f), 7, 5)
    Q = np.zeros((7, n))
    Q[:, f] = Qf.T
    c = _context(key)
    lam, X, info = c.modes_many(6, locked=Q, rtol=RTOL, maxit=3000)
    c.close()
    ref, _ = MU.restricted_truth(Kf, Mf, Qf)
    Qo = np.zeros((7, n))
    Qo[:, f] = MU.m_orthonormalise(Qf, Mf).T
    _check_set(key, lam, X, info, ref[:6], cond, MU.dense_spectrum(key)[3], Q=Qo, restricted=True)
    assert info["batches"] == 1 and info["nOutOfOrder"] == 0


# ---------------------------------------------------------------- continuation
@pytest.mark.parametrize("precond", ["jacobi", "two-level", "multigrid"])
def test_continuation(precond):
    """modes(8), then modes_many(8, locked=X): eigenvalues 9 .. 16 of the dense spectrum."""
    key = (3, 2)
    c = _context(key, precond)
    lam0, X0, _ = c.modes(8, rtol=RTOL, maxit=3000)
    lam, X, info = c.modes_many(8, locked=X0, rtol=RTOL, maxit=3000)
    c.close()
    ref, _, cond, defect_ref = MU.dense_spectrum(key)
    _check_set(key, lam, X, info, ref[8:16], cond, defect_ref, Q=X0)
    both = np.concatenate([X0, X])
    Mm = _device_pencil(key)[1]
    assert np.abs(both @ (Mm @ both.T) - np.eye(16)).max() <= max(10 * defect_ref, both.shape[1] * EPS)


# ---------------------------------------------------------------- sweeps
@functools.lru_cache(maxsize=None)
def _sweep(key, nev, batch, precond, free=False):
    c = _context(key, precond, clamp=not free)
    out = c.modes_many(nev, free=free, batch=batch, rtol=RTOL, maxit=3000)
    c.close()
    return out


SWEEPS = [((3, 2), 48, 16, "multigrid"), ((3, 2), 48, 7, "multigrid"), ((2, 2), 40, 16, "jacobi"), ((2, 2), 40, 7, "jacobi")]


@pytest.mark.parametrize("key,nev,batch,precond", SWEEPS, ids=lambda v: _name(v) if isinstance(v, tuple) else str(v))
def test_sweep(key, nev, batch, precond):
    """The whole sorted list against dense eigh, one to one."""
    lam, X, info = _sweep(key, nev, batch, precond)
    ref, _, cond, defect_ref = MU.dense_spectrum(key)
    _check_set(key, lam, X, info, ref[:nev], cond, defect_ref)
    assert info["batches"] == -(-nev // batch) and info["nOutOfOrder"] == 0


def test_free_free():
    """(3,2) free, 30 modes in batches of 10: the dense non-zero spectrum, M-orthogonal to the rigid modes."""
    key, nev = (3, 2), 30
    lam, X, info = _sweep(key, nev, 10, "multigrid", True)
    ref, _, cond, defect_ref = MU.dense_spectrum(key, True)
    Mm = U.pencil(key)[1]
    Z = U.m_orthonormalise(U.rigid_modes(U.fem_mesh(key).node_pos), Mm)
    _check_set(key, lam, X, info, ref[6:6 + nev], cond, defect_ref, Q=Z.T, free=True)
    assert info["batches"] == 3


def test_multiplicity_across_a_batch_edge():
    """The bar clamped at z = min has exact double eigenvalues at (0,1), (3,4), (7,8), (10,11), ...; batch = 8 cuts the pair (7,8). Eigenvalues
    against the dense list; the two members of the cut pair, found in different batches, span the dense pair's invariant subspace: the
    M-orthogonal projector onto the dense pair leaves them unchanged up to the angle the residual allows, sqrt(cond M) rtol lambda / gap."""
    key = U.BAR
    lam, X, info = _sweep(key, 24, 8, "jacobi")
    ref, Xd, cond, defect_ref = MU.dense_spectrum(key)
    assert abs(ref[8] - ref[7]) <= 1e-9 * ref[7], "the fixture's pair (7, 8) is not double"
    _check_set(key, lam, X, info, ref[:24], cond, defect_ref)
    Kf, Mf, f, _ = MU.dense_clamped(key)
    pair = Xd[:, 7:9]
    gap = min(ref[7] - ref[6], ref[9] - ref[8])
    angle = np.sqrt(cond) * RTOL * ref[8] / gap
    for j in (7, 8):
        x = X[j, f]
        out = x - pair @ (pair.T @ (Mf @ x))
        sin = np.sqrt(out @ (Mf @ out))
        print("mode %d: sine of the angle to the dense pair %.3e (bar %.3e)" % (j, sin, angle))
        assert sin <= angle
    assert info["batches"] == 3 and info["nOutOfOrder"] == 0           # the second member of the cut pair is no missed mode


def test_band():
    """lambda_max in the middle of a gap: nFound = the dense count below it, bandExhausted = 1; with nev below that count bandExhausted = 0."""
    key = (3, 2)
    ref, _, cond, defect_ref = MU.dense_spectrum(key)
    cut = 21                                             # the band holds 21 modes: two batches of 8 do not exhaust it, the third does
    lam_max = 0.5 * (ref[cut - 1] + ref[cut])
    c = _context(key, "multigrid")
    lam, X, info = c.modes_many(64, lambda_max=lam_max, batch=8, rtol=RTOL, maxit=3000)
    assert info["nFound"] == cut == len(lam) and info["bandExhausted"] == 1 and info["batches"] == 3
    _check_set(key, lam, X, info, ref[:cut], cond, defect_ref)
    lam2, X2, info2 = c.modes_many(16, lambda_max=lam_max, batch=8, rtol=RTOL, maxit=3000)
    assert info2["nFound"] == 16 and info2["bandExhausted"] == 0 and info2["batches"] == 2
    _check_set(key, lam2, X2, info2, ref[:16], cond, defect_ref)
    c.close()


def test_mid_mesh():
    """8 x 7 x 6 quadratic tets, multigrid, 30 modes in batches of 12 against shift-invert eigsh: the only case whose kernels span many workgroups."""
    key, nev = U.MID, 30
    lam, X, info = _sweep(key, nev, 12, "multigrid")
    ref, _, cond, defect_ref = U.clamped_truth(key, 34)
    _check_set(key, lam, X, info, ref[:nev], cond, defect_ref)
    assert info["batches"] == 3 and info["precondUsed"] == M.PRECOND_MULTIGRID and info["nOutOfOrder"] == 0


# ---------------------------------------------------------------- identity, state
@pytest.mark.parametrize("free", [False, True], ids=["clamped", "free"])
def test_one_batch_is_mfh_modes(free):
    key = (3, 2)
    c = _context(key, "multigrid", (("deterministic", 1),), clamp=not free)
    l1, X1, i1 = c.modes(5, free=free, rtol=RTOL)
    l2, X2, i2 = c.modes_many(5, free=free, rtol=RTOL)
    c.close()
    assert np.array_equal(l1, l2) and np.array_equal(X1, X2) and np.array_equal(i1["residuals"], i2["residuals"])
    assert i2["batches"] == 1 and i2["iterations"] == i1["iterations"] and i2["nFound"] == 5


def _probe(c):
    n = c.bs * c.n_dof
    rng = np.random.default_rng(5)
    f, x = rng.standard_normal(n), rng.standard_normal(n)
    u = c.solve(f, rtol=1e-9)
    return u, c.apply_K(x), c.export_upper_triplets()


def test_nothing_existing_moves():
    """After a modes_many call, solve, K x, export and modes(3) are bit-identical to a fresh context's (the check of
    tests/test_gpu_modes.py::test_nothing_existing_moves, on the default storage, which the call widens for its duration); two modes_many calls
    return the same bits."""
    key = (3, 2)
    opts = (("deterministic", 1),)
    a = _context(key, "multigrid", opts)
    l1, X1, info = a.modes_many(20, batch=8, rtol=RTOL)
    assert "both triangles" in info["note"] and info["batches"] == 3
    got = _probe(a)
    b = _context(key, "multigrid", opts)
    want = _probe(b)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for g, w_ in zip(got[2], want[2]):
        assert np.array_equal(g, w_)
    la, Xa, _ = a.modes(3, rtol=RTOL)
    lb, Xb, _ = b.modes(3, rtol=RTOL)
    assert np.array_equal(la, lb) and np.array_equal(Xa, Xb)
    l2, X2, info2 = a.modes_many(20, batch=8, rtol=RTOL)
    assert np.array_equal(l1, l2) and np.array_equal(X1, X2) and np.array_equal(info["residuals"], info2["residuals"])
    a.close(); b.close()


# ---------------------------------------------------------------- limits
def test_maxit_two():
    key = (3, 2)
    c = _context(key, "jacobi")
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes_many(12, batch=6, rtol=RTOL, maxit=2)
    assert ei.value.code == _lib.ERR_NOT_CONVERGED
    lam, X, info = c.last_modes_many
    assert info["converged"] == 0 and info["batches"] == 1 and info["iterations"] == 2 and info["nFound"] == 6 == len(lam)
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(X)) and np.all(lam > 0) and np.all(np.diff(lam) >= 0)
    assert np.all(np.isfinite(info["residuals"])) and info["maxResidual"] > RTOL
    n = c.bs * c.n_dof
    u = c.solve(np.ones(n), rtol=1e-8)
    assert c.last_info["converged"] == 1 and np.all(np.isfinite(u))
    c.close()


def test_rank_deficient_locked_set():
    key = (3, 1)
    c = _context(key)
    n = c.bs * c.n_dof
    Q = np.random.default_rng(2).standard_normal((30, n))
    for rows in ([0, 1, 2, 1], list(range(30)) + [3]):            # a repeated row inside one group of 24, and one across two groups
        bad = Q[rows].copy()
        if len(rows) > 24:
            bad[-1] = 0.5 * Q[3] - 2.0 * Q[7]
        with pytest.raises(M.MeshFEMHipError) as ei:
            c.modes_many(2, locked=bad, rtol=RTOL)
        assert ei.value.code == _lib.ERR_INVALID and "rank deficient" in str(ei.value)
    # rows that live on the clamp only are zero on the pencil
    only_clamp = np.zeros((1, n))
    only_clamp[0, U.clamp_vars(key)] = 1.0
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes_many(2, locked=only_clamp, rtol=RTOL)
    assert ei.value.code == _lib.ERR_INVALID
    # the context works on
    lam, X, info = c.modes_many(2, locked=Q[:3], rtol=RTOL, maxit=3000)
    assert info["converged"] == 1
    c.close()


def test_counts_beyond_the_pencil_and_device_side_refusals():
    key = (2, 1)
    c = _context(key)
    n = c.bs * c.n_dof
    n_eff = n - len(U.clamp_vars(key))
    assert n_eff < 256
    Q = np.random.default_rng(1).standard_normal((5, n))
    for kw in (dict(nev=n_eff + 1), dict(nev=n_eff - 4, locked=Q)):
        with pytest.raises(M.MeshFEMHipError) as ei:
            c.modes_many(kw.pop("nev"), **kw)
        assert ei.value.code == _lib.ERR_INVALID
    # what mfh_modes refuses: the free case on a clamped context, a clamp that leaves rigid motions free, another operator, a DoF map in the free case
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes_many(2, free=True)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    c.clear_fixed()
    c.fix_variables([0, 1])
    with pytest.raises(M.MeshFEMHipError, match="rigid motions free") as ei:
        c.modes_many(2)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    c.set_operator(M.OP_MASS_VECTOR)
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes_many(2)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    c.close()
    c = _context(U.BAR, clamp=False)
    assert c.apply_periodic_conditions() < c.n_node
    with pytest.raises(M.MeshFEMHipError) as ei:
        c.modes_many(2, free=True)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    c.close()


# ---------------------------------------------------------------- Simulator layer
def _cantilever():
    import json
    from meshfem_amd import grid
    from meshfem_amd.linear_elasticity import Simulator
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cantilever")
    bc = json.load(open(os.path.join(gold, "cantilever.bc")))
    mat = json.load(open(os.path.join(gold, "B9Creator.material")))
    box = [r for r in bc["regions"] if r["type"] == "dirichlet"][0]["box%"]
    V, T = grid.grid_tet_mesh(20, 4, 4)
    sim = Simulator(T, V, 1)
    sim.ctx.set_preconditioner(M.PRECOND_MULTIGRID)
    sim.setIsotropicMaterial(mat["young"], mat["poisson"])
    sim.applyDirichletBox(box["minCorner"], box["maxCorner"], [0, 0, 0], relative=True)
    return sim, mat


def _exported_pencil(ctx, fixed, density):
    """(Kff, Mff, free variables, M) of a context's own exported pencil as scipy CSR, M = density x the exported mass matrix."""
    n = ctx.bs * ctx.n_dof
    out = []
    for op in (M.OP_ELASTICITY, M.OP_MASS_VECTOR):
        ctx.set_operator(op)
        ctx.assemble()
        i, j, v = ctx.export_upper_triplets()
        U_ = sp.coo_matrix((v, (i.astype(np.int64), j.astype(np.int64))), shape=(n, n)).tocsr()
        out.append(sp.csr_matrix(U_ + sp.triu(U_, 1).T))
    ctx.set_operator(M.OP_ELASTICITY)
    keep = np.ones(n, dtype=bool)
    keep[fixed] = False
    f = np.nonzero(keep)[0]
    Mfull = density * out[1]
    return out[0][f][:, f], Mfull[f][:, f], f, Mfull


def test_simulator_band_on_the_golden_cantilever():
    """vibrational_modes_many(fmax=...) on tests/golden/cantilever (20 x 4 x 4 linear tets, 1 575 unknowns): all natural frequencies below fmax,
    against shift-invert eigsh on the exported pencil."""
    sim, mat = _cantilever()
    fixed, _ = sim.ctx.bc_dirichlet_vars()
    Kf, Mf, f, _ = _exported_pencil(sim.ctx, fixed, mat["density"])
    lam, _ = U.shift_invert_eigsh(Kf, Mf, 0.0, 20)
    freq_ref = np.sqrt(lam) / (2 * np.pi)
    # the band ends in the first gap of more than 1 % past a dozen modes (the square section has near-double bending modes): two batches of 8
    cut = next(k for k in range(12, 16) if freq_ref[k] - freq_ref[k - 1] > 0.01 * freq_ref[k])
    fmax = 0.5 * (freq_ref[cut - 1] + freq_ref[cut])
    freq, modes = sim.vibrational_modes_many(fmax=fmax, density=mat["density"], batch=8, rtol=RTOL)
    info = sim.modes_many_info
    print("cantilever: %d frequencies below %.4g Hz in %d batches, %d iterations" % (len(freq), fmax, info["batches"], info["iterations"]))
    assert info["converged"] == 1 and info["bandExhausted"] == 1 and len(freq) == cut and modes.shape == (cut, sim.numNodes(), 3)
    cond = U.cond_of_mass(Mf)
    # d f / f = d lambda / (2 lambda)
    assert np.all(np.abs(freq - freq_ref[:cut]) <= 0.5 * np.sqrt(cond) * RTOL * freq_ref[:cut])
    sim.ctx.close()


def test_simulator_modes_for_mass_fraction():
    """modesForMassFraction(0.9) on the bar clamped at z = min: the mode count and the fractions against the same quantities from the dense
    eigenvectors -- cumulative (x_j^T M r_d)^2 over r_f^T M_ff r_f per direction, the first count (a multiple of the batch) at which all three
    reach 0.9."""
    from meshfem_amd.linear_elasticity import Simulator
    V, T, deg, _ = U.mesh_arrays(U.BAR)
    sim = Simulator(T, V, deg)
    sim.setIsotropicMaterial(U.E_MOD, U.NU)
    lo, hi = V.min(axis=0), V.max(axis=0)
    sim.applyDirichletBox([lo[0] - 1, lo[1] - 1, lo[2] - 1e-9], [hi[0] + 1, hi[1] + 1, lo[2] + 1e-9], [0, 0, 0])
    fixed, _ = sim.ctx.bc_dirichlet_vars()
    assert np.array_equal(np.sort(fixed), np.sort(U.clamp_vars(U.BAR, 2)))
    import scipy.linalg
    Kf, Mf, f, Mfull = (a if isinstance(a, np.ndarray) else a.toarray() for a in _exported_pencil(sim.ctx, fixed, 1.0))
    lam, Xd = scipy.linalg.eigh(Kf, Mf)
    n = Mfull.shape[0]
    batch = 6
    eff, total = np.zeros((len(lam), 3)), np.zeros(3)
    for d in range(3):
        r = np.zeros(n)
        r[d::3] = 1.0
        eff[:, d] = (Xd.T @ (Mfull @ r)[f]) ** 2
        r[fixed] = 0.0
        total[d] = r @ (Mfull @ r)
    cum = np.cumsum(eff, axis=0) / total[None, :]
    count = next(k for k in range(batch, len(lam) + 1, batch) if np.all(cum[k - 1] >= 0.9))
    # the count must not hinge on rounding: the fractions one batch earlier are clearly short, those at the count clearly there
    assert cum[count - batch - 1].min() < 0.9 - 1e-3 and cum[count - 1].min() > 0.9 + 1e-3
    freq, modes, frac = sim.modesForMassFraction(0.9, batch=batch, rtol=RTOL)
    print("bar: %d modes for 90 %% of the mass, fractions %s (dense %s)" % (len(freq), frac, cum[count - 1]))
    assert len(freq) == count and modes.shape == (count, sim.numNodes(), 3)
    # The summed effective mass of the first `count` modes is |P M r|^2 in the M^-1 norm, P the M-orthogonal projector onto their span: it moves
    # by at most 2 sin(theta) |M r|^2, theta the angle between the computed span and the true one, sin(theta) <= sqrt(cond M) rtol lambda / gap
    # with the gap to mode count + 1 (3 % on this fixture; the double modes inside the span play no part in the sum)
    cond = np.linalg.cond(Mf)
    gap = lam[count] - lam[count - 1]
    assert gap >= 0.01 * lam[count - 1]
    bar = 2.0 * np.sqrt(cond) * RTOL * lam[count - 1] / gap * eff.sum(axis=0) / total
    assert np.all(np.abs(frac - cum[count - 1]) <= bar)
    fr = np.sqrt(lam[:count]) / (2 * np.pi)
    assert np.all(np.abs(freq - fr) <= 0.5 * np.sqrt(cond) * RTOL * fr)
    # nmax stops the loop
    freq2, _, frac2 = sim.modesForMassFraction(0.9, nmax=batch, batch=batch, rtol=RTOL)
    assert len(freq2) == batch and frac2.min() < 0.9
    sim.ctx.close()
