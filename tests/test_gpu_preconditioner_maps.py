"""The preconditioners of the PCG as linear maps z = M^-1 r, through the test hook mfh_debug_apply_precond (the preconditioner the next
solve uses, ungated): block-Jacobi, two-level and the multigrid V-cycle in its variants. PCG needs M symmetric positive definite and
FIXED (the same linear map at every iteration); a V-cycle whose restriction is not the transpose of its prolongation, or a work vector
that is not re-zeroed between applications, still converges -- only more slowly -- so the solve tests do not notice. Checked here:

- block-Jacobi equals the inverse diagonal blocks of the oracle's K (fixed components decoupled), 1e-13 relative;
- symmetric: |y . Mx - x . My| <= tau |x| |Mx| for 8 random pairs. Measured on the MI355X (first run of this file): at most 1.0e-16
  with FP64 storage (block-Jacobi: the blocks are stored symmetrized by k_diag_inv; two-level; multigrid with mg_coarse_fp32 0) and at
  most 2.1e-16 with the default FP32 copies of the multigrid levels (both smoothing sweeps read the same rounded matrix, and the two
  triangles of K round alike), so one bound serves both: tau = 1e-13, tighter than the 1e-11 / 1e-6 an FP64 / FP32 budget allows;
- positive: x . Mx > 0 for random vectors and for the rigid-body modes restricted to the free rows;
- linear: M(a x + b y) = a Mx + b My to 1e-12;
- stable: two applications agree to rounding (1e-13), bit for bit with option deterministic 1;
- the batched applications (multigrid: the batched V-cycle, 3D NR 2 and 6, 2D NR 3; two-level: k_tl_*_nr) equal NR single ones to 1e-12.

All inputs are zero on the fixed rows and the comparisons run over the free rows."""
import numpy as np
import pytest
import scipy.sparse as sp

import meshfem_amd as M
from meshfem_amd import _lib as L
from meshfem_amd import grid
from oracle import c_oracle as CO
from oracle import meshfem_oracle as O

pytestmark = pytest.mark.gpu

TAU_FP64 = 1e-13
TAU_FP32 = 1e-13
BATCHES = {3: (2, 6), 2: (3,)}

MG_VARIANTS = {
    "mg_default": {},
    "mg_deep": {"mg_agg_target": 6, "mg_dense_max": 8},        # several aggregate (stencil) levels
    "mg_dense_only": {"mg_dense_max": 100000},                  # the first aggregate level is the dense one
    "mg_coarse_cycles2": {"mg_coarse_cycles": 2},
    "mg_steps2": {"mg_steps_fine": 2, "mg_steps_coarse": 2},
    "mg_fp64": {"mg_coarse_fp32": 0},
}
KINDS = ["block_jacobi", "two_level"] + list(MG_VARIANTS)


def _mesh(dim, seed=0):
    if dim == 3:
        V, T = grid.grid_tet_mesh(6, 5, 4)
    else:
        V, T = grid.grid_tri_mesh(20, 16)
    V = np.array(V, dtype=np.float64)
    lo, hi = V.min(axis=0), V.max(axis=0)
    inner = np.all((V > lo + 1e-9) & (V < hi - 1e-9), axis=1)
    rng = np.random.default_rng(seed + dim)
    V[inner] += 0.04 * rng.uniform(-1.0, 1.0, size=(inner.sum(), dim))
    return V, np.asarray(T)


def _setup(dim, deg, bc, kind, extra=()):
    """(context, fixed-row mask, DoF positions); material: an isotropic field (E varies by 6x)."""
    V, T = _mesh(dim)
    rng = np.random.default_rng(21)
    E, nu = rng.uniform(50.0, 300.0, len(T)), rng.uniform(0.1, 0.4, len(T))
    c = M.Context(0)
    for k, v in extra:
        c.set_option(k, v)
    opts = MG_VARIANTS.get(kind, {})
    for k, v in opts.items():
        c.set_option(k, v)
    c.mesh_build(T, V, deg)
    c.material_iso_field(E, nu)
    pos = c.node_positions()
    if bc == "periodic":
        c.apply_periodic_conditions()
        dof = c.get_dof_map()[0]
        dofs = np.array([dof[c.pin_node()]])
    else:
        dof = np.arange(c.n_node)
        dofs = np.unique(np.nonzero(pos[:, 0] < V[:, 0].min() + 1e-9)[0])
    var = (dofs[:, None] * dim + np.arange(dim)).ravel()
    c.fix_variables(var, np.zeros(len(var)))
    fixed = np.zeros(dim * c.n_dof, bool)
    fixed[var] = True
    dpos = np.zeros((c.n_dof, dim))
    dpos[dof[::-1]] = pos[::-1]                # a DoF's position: that of its first node
    c.set_preconditioner({"block_jacobi": M.PRECOND_BLOCK_JACOBI, "two_level": M.PRECOND_TWO_LEVEL}.get(kind, M.PRECOND_MULTIGRID))
    return c, fixed, dpos, (V, T, E, nu, dof if bc == "periodic" else None)


def _rigid_modes(dpos, dim):
    n = len(dpos)
    modes = []
    for a in range(dim):
        m = np.zeros((n, dim))
        m[:, a] = 1.0
        modes.append(m.ravel())
    rots = [(0, 1)] if dim == 2 else [(0, 1), (1, 2), (2, 0)]
    for a, b in rots:
        m = np.zeros((n, dim))
        m[:, a], m[:, b] = -dpos[:, b], dpos[:, a]
        modes.append(m.ravel())
    return modes


def _apply(c, R):
    return c.debug_apply_precond(R)


def _check_map(c, fixed, dpos, dim, tau, rng, deterministic=False):
    n = len(fixed)
    free = ~fixed

    def rnd(k=1):
        X = rng.standard_normal((k, n))
        X[:, fixed] = 0.0
        return X
    # symmetric, positive
    worst = 0.0
    for _ in range(8):
        x, y = rnd()[0], rnd()[0]
        Mx, My = _apply(c, x)[0], _apply(c, y)[0]
        asym = abs(y[free] @ Mx[free] - x[free] @ My[free]) / (np.linalg.norm(x) * np.linalg.norm(Mx[free]))
        worst = max(worst, asym)
        assert x[free] @ Mx[free] > 0 and y[free] @ My[free] > 0
    assert worst <= tau, "asymmetry %.3e > %.1e" % (worst, tau)
    for m in _rigid_modes(dpos, dim):
        m[fixed] = 0.0
        assert m[free] @ _apply(c, m)[0][free] > 0
    # linear
    x, y = rnd()[0], rnd()[0]
    a, b = 1.7, -0.6
    Mx, My, Mxy = _apply(c, x)[0], _apply(c, y)[0], _apply(c, a * x + b * y)[0]
    lin = np.linalg.norm((Mxy - a * Mx - b * My)[free]) / (abs(a) * np.linalg.norm(Mx[free]) + abs(b) * np.linalg.norm(My[free]))
    assert lin <= 1e-12, "nonlinear: %.3e" % lin
    # stable
    Mx2 = _apply(c, x)[0]
    if deterministic:
        assert np.array_equal(Mx2, Mx), "deterministic 1: two applications differ"
    else:
        assert np.linalg.norm((Mx2 - Mx)[free]) <= 1e-13 * np.linalg.norm(Mx[free])
    return worst


CASES = [(dim, deg, bc, kind) for dim, deg in ((3, 2), (3, 1), (2, 2), (2, 1)) for bc in ("dirichlet", "periodic") for kind in KINDS
         if not (deg == 1 and kind in ("mg_dense_only",))]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dim,deg,bc,kind", CASES)
def test_preconditioner_is_a_fixed_spd_map(dim, deg, bc, kind):
    c, fixed, dpos, _ = _setup(dim, deg, bc, kind)
    rng = np.random.default_rng(3)
    r = rng.standard_normal(len(fixed))
    r[fixed] = 0.0
    _apply(c, r)                                 # builds the preconditioner
    if kind.startswith("mg"):
        levels = c.multigrid_levels()
        if kind == "mg_default":
            assert len(levels) >= 1, levels
        if kind == "mg_deep":
            assert len(levels) >= 2, levels
    tau = TAU_FP64 if kind in ("block_jacobi", "two_level", "mg_fp64") else TAU_FP32
    worst = _check_map(c, fixed, dpos, dim, tau, rng)
    print("%s %dD P%d %s: asymmetry %.2e" % (kind, dim, deg, bc, worst))
    # batched == single
    if kind == "two_level" or (kind.startswith("mg") and deg == 2):
        for nr in BATCHES[dim]:
            R = rng.standard_normal((nr, len(fixed)))
            R[:, fixed] = 0.0
            Zb = _apply(c, R)
            for k in range(nr):
                z = _apply(c, R[k])[0]
                err = np.linalg.norm((Zb[k] - z)[~fixed]) / np.linalg.norm(z[~fixed])
                assert err <= 1e-12, "%s nr=%d k=%d: batched vs single %.3e" % (kind, nr, k, err)
    elif kind == "block_jacobi" or (kind.startswith("mg") and deg == 1):
        with pytest.raises(M.MeshFEMHipError) as ei:
            _apply(c, np.zeros((BATCHES[dim][-1], len(fixed))))
        assert ei.value.code == L.ERR_UNSUPPORTED
    c.close()


@pytest.mark.parametrize("bc", ["dirichlet", "periodic"])
@pytest.mark.parametrize("dim,deg", [(3, 2), (3, 1), (2, 2), (2, 1)])
def test_block_jacobi_is_the_inverse_diagonal_blocks(dim, deg, bc):
    """z = B_i^-1 r_i per DoF block of the oracle's K, the fixed components decoupled (identity), 1e-13 relative."""
    c, fixed, dpos, (V, T, E, nu, dof) = _setup(dim, deg, bc, "block_jacobi")
    D = np.stack([O.ElasticityTensor.isotropic(dim, a, b).D for a, b in zip(E, nu)])
    Ap, Ai, Ax, _ = CO.assemble_csc(dim, deg, c.elem_nodes(), V, D, c.n_dof, dof)
    n = dim * c.n_dof
    U = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n))
    K = (U + U.T - sp.diags(U.diagonal())).tocsr()
    r = np.random.default_rng(8).standard_normal(n)
    r[fixed] = 0.0
    z = _apply(c, r)[0]
    zref = np.zeros(n)
    for q in range(c.n_dof):
        ix = np.arange(q * dim, (q + 1) * dim)
        f = ix[~fixed[ix]]
        if len(f):
            B = K[f][:, f].toarray()
            zref[f] = np.linalg.solve(B, r[f])
    free = ~fixed
    err = np.abs(z - zref)[free].max()
    assert err <= 1e-13 * np.abs(zref[free]).max(), err
    c.close()


@pytest.mark.parametrize("kind", ["block_jacobi", "two_level", "mg_default"])
@pytest.mark.parametrize("dim,deg", [(3, 2), (2, 1)])
def test_deterministic_preconditioner_is_bitwise_stable(dim, deg, kind):
    """Option deterministic 1: the same properties, and two applications bit-identical."""
    c, fixed, dpos, _ = _setup(dim, deg, "dirichlet", kind, (("deterministic", 1),))
    tau = TAU_FP64 if kind != "mg_default" else TAU_FP32
    _check_map(c, fixed, dpos, dim, tau, np.random.default_rng(12), deterministic=True)
    c.close()
