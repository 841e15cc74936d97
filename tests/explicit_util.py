"""Shared helpers of the explicit-dynamics tests (tests/test_explicit_reference.py, tests/test_gpu_explicit.py): numpy
restatements, on the oracle's matrices and the meshes of tests/modes_util.py, of
  - HRZ lumping: m_d = sum over the (element, local node) pairs of DoF d of rho_e vol_e Mref_ii / trace(Mref), Mref from the oracle's quadrature;
  - the two bounds of mfh_explicit_dt: the Gershgorin bound from the oracle's element stiffness matrices and the power iteration;
  - the recurrence of mfh_explicit, in float64 and in np.longdouble:
        v(n+1/2) = v(n) + dt/2 a(n),  u(n+1) = u(n) + dt v(n+1/2),
        a(n+1) = (M_L^-1 (g(n+1) f - K u(n+1)) - aR v(n+1/2)) / (1 + aR dt/2),  v(n+1) = v(n+1/2) + dt/2 a(n+1),
    a(0) = M_L^-1 (g(0) f - K u(0)) - aR v(0), fixed variables held at zero.
The library's reference project has no time integrator, so this recurrence is the independent reference. The bars of the device tests are multiples
of the recurrence's own float64-versus-longdouble defect, measured here (the margin policy of docs/design/04_13_dynamics.md). Every reference is
computed once per process (functools.lru_cache) and handed out read-only."""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import meshfem_oracle as O

import modes_util as U

DENSITY = 1.7
ALPHA_REL = 0.1            # the damped cases: aR = ALPHA_REL omega_1
LD = np.longdouble


def name(key):
    return key if isinstance(key, str) else "%dD-P%d" % key


@functools.lru_cache(maxsize=None)
def mref(key):
    """The consistent mass matrix of the unit-volume element: the quadrature MassMatrix::construct uses (oracle.mass_triplets)."""
    m = U.fem_mesh(key)
    pts, w = O.quadrature_rule(m.K, 2 * m.deg)
    Phi = np.array([O.shape_functions(m.deg, m.K, p) for p in pts])
    return np.einsum('q,qi,qj->ij', w, Phi, Phi)


def hrz_weights(key):
    M = mref(key)
    return np.diag(M) / np.trace(M)


@functools.lru_cache(maxsize=None)
def volumes(key):
    vol, _ = U.fem_mesh(key).embeddings_batch()
    return np.asarray(vol, dtype=np.float64)


def element_density(key, seed=None):
    """None (unit density) or a random positive field."""
    if seed is None:
        return None
    return 0.5 + np.random.default_rng(seed).random(len(volumes(key)))


@functools.lru_cache(maxsize=None)
def exact_weights(key):
    """The HRZ weights as fractions: the entries of the element mass matrix are rationals with small denominators, which the oracle's quadrature
    returns to a few eps (its points and weights are float64 numbers); snapping them makes the restatement exact where the quadrature is not."""
    from fractions import Fraction
    d = [Fraction(float(x)).limit_denominator(100000) for x in np.diag(mref(key))]
    assert all(abs(float(q) / x - 1) <= 64 * U.EPS for q, x in zip(d, np.diag(mref(key))))
    tr = sum(d)
    return tuple(q / tr for q in d)


def lumped_mass(key, rho=None, vol=None, w=None):
    """(m [n_node * dim] in np.longdouble, pairs per node): the pairs of a node are added in ascending element order, the order of the library's
    pair list. vol, w: the element volumes and the weights (default: the oracle's volumes and the exact weights; a device test passes the
    library's own, which differ from them in the last bits and are checked apart)."""
    m = U.fem_mesh(key)
    w = np.array([LD(q.numerator) / LD(q.denominator) for q in exact_weights(key)], dtype=LD) if w is None else np.asarray(w, dtype=np.float64).astype(LD)
    vol = volumes(key) if vol is None else np.asarray(vol, dtype=np.float64)
    rv = vol.astype(LD) if rho is None else np.asarray(rho, dtype=np.float64).astype(LD) * vol.astype(LD)
    contrib = rv[:, None] * w[None, :]
    out = np.zeros(m.num_nodes, dtype=LD)
    np.add.at(out, m.elem_nodes.reshape(-1), contrib.reshape(-1))          # (sequential, element-major: ascending element per node)
    count = np.bincount(m.elem_nodes.reshape(-1), minlength=m.num_nodes)
    return np.repeat(out, m.N), np.repeat(count, m.N)


@functools.lru_cache(maxsize=None)
def elem_abs_rowsums(key, mode="iso"):
    """[n_elem, npe, dim]: sum_j |K_e[(i, c), j]| of the oracle's element stiffness matrices. mode: "iso" (E = 1, nu = 0.3, the material of every
    other reference here) or a material mode of tests/element_integrals_util.py (general, ortho_field, general_field, ...): the tensors it returns."""
    V, T, deg, _ = U.mesh_arrays(key)
    m = U.fem_mesh(key)
    sim = O.Simulator(T, V, deg, mesh=m)
    if mode == "iso":
        sim.set_material_constant(O.ElasticityTensor.isotropic(m.N, U.E_MOD, U.NU))
    else:
        import element_integrals_util as EI
        D = EI.material(mode, m.N, len(T))[1]
        if D.ndim == 2:
            sim.set_material_constant(O.ElasticityTensor(m.N, D))
        else:
            sim.set_material_field([O.ElasticityTensor(m.N, De) for De in D])
    Ke = sim.per_element_stiffness()
    return np.abs(Ke).sum(axis=2).reshape(len(Ke), m.nodes_per_elem, m.N)


def lambda_upper(key, fixed, density=1.0, rho=None):
    """max over the free variables of (sum over the pairs of the absolute element row sums) / (density m)."""
    m = U.fem_mesh(key)
    rs = elem_abs_rowsums(key)
    acc = np.zeros((m.num_nodes, m.N))
    np.add.at(acc, m.elem_nodes.reshape(-1), rs.reshape(-1, m.N))
    g = acc.reshape(-1) / lumped_mass(key, rho)[0].astype(np.float64)
    keep = np.ones(g.size, dtype=bool)
    keep[np.asarray(fixed, dtype=np.int64)] = False
    return float(g[keep].max() / density)


def default_start(n):
    """The default start vector of mfh_explicit_dt."""
    i = np.arange(1, n + 1, dtype=np.uint64)
    return (((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5


class CsrLD:
    """y = K x for a scipy CSR matrix in any floating type (scipy's own product does not take np.longdouble)."""

    def __init__(self, K, dtype):
        K = sp.csr_matrix(K)
        K.sort_indices()
        assert np.all(np.diff(K.indptr) > 0)
        self.data, self.indices, self.starts = K.data.astype(dtype), K.indices, K.indptr[:-1]

    def __call__(self, x):
        return np.add.reduceat(self.data * x[self.indices], self.starts)


def matvec(K, dtype):
    if dtype == np.float64:
        Kc = sp.csr_matrix(K)
        return lambda x: Kc @ x
    return CsrLD(K, dtype)


def power_iteration(K, mass, fixed, x0, iters=60, dtype=np.float64):
    """The power iteration of mfh_explicit_dt as the device runs it: with s = 1 / sqrt(x . M x), xn = s x, yn = s K x: lam = xn . yn, x <- M^-1 yn."""
    mv = matvec(K, dtype)
    mass = np.asarray(mass).astype(dtype)
    inv = 1.0 / mass
    inv[np.asarray(fixed, dtype=np.int64)] = 0.0
    keep = (inv != 0).astype(dtype)
    x = np.asarray(x0).astype(dtype) * keep
    nrm = np.sum(mass * x * x)
    lam = dtype(0)
    for _ in range(iters):
        y = mv(x) * keep
        s = 1.0 / np.sqrt(nrm)
        yn, xn = s * y, s * x
        lam = np.sum(xn * yn)
        x = inv * yn
        nrm = np.sum(x * yn)
    return lam


def explicit_direct(K, mass, fixed, dt, n_steps, u0, v0, f=None, amplitude=None, alpha=0.0, a0=None, dtype=np.float64):
    """The recurrence on full-length vectors. mass: density x the lumped masses, one per variable. Returns (U, V, A, E): the states of the steps
    0 .. n_steps and the energies [n_steps + 1, 4] = 1/2 v.Mv, 1/2 u.Ku, g f.u, 1/2 v(n+1/2).M v(n+1/2) + 1/2 u(n+1).K u(n)."""
    mv = matvec(K, dtype)
    n = K.shape[0]
    mass = np.asarray(mass).astype(dtype)
    inv = 1.0 / mass
    inv[np.asarray(fixed, dtype=np.int64)] = 0.0
    keep = (inv != 0).astype(dtype)
    dt, alpha = dtype(dt), dtype(alpha)
    hdt, den = dt / 2, 1 + alpha * (dt / 2)
    g = np.ones(n_steps + 1, dtype=dtype) if amplitude is None else np.asarray(amplitude).astype(dtype)
    ff = np.zeros(n, dtype=dtype) if f is None else np.asarray(f).astype(dtype)
    u, v = np.asarray(u0).astype(dtype) * keep, np.asarray(v0).astype(dtype) * keep
    y = mv(u) * keep
    a = inv * (g[0] * ff - y) - alpha * v if a0 is None else np.asarray(a0).astype(dtype) * keep
    Us, Vs, As = (np.zeros((n_steps + 1, n), dtype=dtype) for _ in range(3))
    E = np.zeros((n_steps + 1, 4), dtype=dtype)
    for k in range(n_steps + 1):
        if k > 0:
            a = (inv * (g[k] * ff - y) - alpha * vh) / den
            v = vh + hdt * a
        vh = v + hdt * a
        un = u + dt * vh
        Us[k], Vs[k], As[k] = u, v, a
        E[k] = 0.5 * np.sum(mass * v * v), 0.5 * np.sum(u * y), g[k] * np.sum(ff * u), 0.5 * (np.sum(mass * vh * vh) + np.sum(un * y))
        if k < n_steps:
            u = un
            y = mv(u) * keep
    return Us, Vs, As, E


# ---- the pencil (K, density M_L) of the fixtures
def fixed_of(key, clamped=True):
    return U.clamp_vars(key) if clamped else np.zeros(0, dtype=np.int64)


def free_of(key, clamped=True):
    return U.free_vars(key, fixed_of(key, clamped))


_DEVICE_MASSES = {}


def register_device_masses(key, m):
    """The lumped masses as the device returned them (mfh_mass_lumped_hrz, checked on its own): a device test runs the recurrence on them, so that
    the stepper is compared on the same pencil and not on masses that differ in the last bits."""
    _DEVICE_MASSES[key] = np.array(m, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def masses(key, source="oracle"):
    """density x the lumped masses at unit density field, per variable. source: "oracle" (the restatement) | "device" (register_device_masses)."""
    m = DENSITY * (lumped_mass(key)[0].astype(np.float64) if source == "oracle" else _DEVICE_MASSES[key])
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def spectrum(key, clamped=True):
    """(lam ascending, Phi columns, full length, M_L-orthonormal) of (K, density M_L) on the free variables: dense on the small meshes; on the mid
    mesh the largest eigenpair alone (Lanczos on M_L^-1/2 K M_L^-1/2)."""
    K = U.pencil(key)[0]
    free = free_of(key, clamped)
    d = 1.0 / np.sqrt(masses(key)[free])
    Kf = K[free][:, free]
    n = K.shape[0]
    if key == U.MID:
        S = sp.diags(d) @ Kf @ sp.diags(d)
        lam, Z = spla.eigsh(S, k=1, which="LA", tol=1e-12)
    else:
        lam, Z = scipy.linalg.eigh(Kf.toarray() * d[:, None] * d[None, :])
    Phi = np.zeros((n, len(lam)))
    Phi[free] = Z * d[:, None]
    return lam, Phi


def lambda_max(key, clamped=True):
    return float(spectrum(key, clamped)[0][-1])


def dt_crit(key, clamped=True):
    return 2.0 / np.sqrt(lambda_max(key, clamped))


def omega1(key, clamped=True):
    lam = spectrum(key, clamped)[0]
    nz = 0 if clamped else (6 if U.fem_mesh(key).N == 3 else 3)
    return float(np.sqrt(lam[nz]))


@functools.lru_cache(maxsize=None)
def case_inputs(key, case, n_steps=200, clamped=True):
    """The inputs of one reference run at dt = 0.9 dt_crit: a random load with a random amplitude table, non-zero u0 and v0 (zero on the clamp).
    case: "undamped" | "damped" (aR = ALPHA_REL x the lowest non-zero frequency; the mid mesh, whose low spectrum is not computed, takes
    aR = 0.01 sqrt(lambda_max))."""
    n = U.pencil(key)[0].shape[0]
    rng = np.random.default_rng(23)
    keep = np.zeros(n)
    keep[free_of(key, clamped)] = 1.0
    w = 0.1 * np.sqrt(lambda_max(key, clamped)) if key == U.MID else omega1(key, clamped)
    f = rng.standard_normal(n) * keep
    u0 = rng.standard_normal(n) * keep
    v0 = w * rng.standard_normal(n) * keep
    amp = rng.standard_normal(n_steps + 1)
    if not clamped:
        # A free body under a random load flies away: its rigid displacement grows like t^2 and soon dominates u, and K times it -- zero but for
        # rounding, and rounded differently by every way of forming K -- then sets the error of a comparison. The load is therefore
        # self-equilibrated and the start state free of linear and angular momentum (test_free_body_keeps_its_momentum covers the flight).
        m = masses(key)
        Z = U.rigid_modes(U.fem_mesh(key).node_pos)
        G = np.linalg.inv(Z.T @ (m[:, None] * Z))
        f = f - m * (Z @ (G @ (Z.T @ f)))
        u0 = u0 - Z @ (G @ (Z.T @ (m * u0)))
        v0 = v0 - Z @ (G @ (Z.T @ (m * v0)))
    d = dict(dt=0.9 * dt_crit(key, clamped), n_steps=n_steps, amplitude=amp, f=f, u0=u0, v0=v0, density=DENSITY,
             alpha=ALPHA_REL * w if case == "damped" else 0.0)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference_run(key, case, n_steps=200, clamped=True, dtype=np.float64, source="oracle"):
    K = U.pencil(key)[0]
    i = case_inputs(key, case, n_steps, clamped)
    out = explicit_direct(K, masses(key, source), fixed_of(key, clamped), i["dt"], n_steps, i["u0"], i["v0"], i["f"], i["amplitude"], i["alpha"], dtype=dtype)
    for a in out:
        a.setflags(write=False)
    return out


def rel_l2_rows(A, B):
    """max over the rows of ||A_k - B_k||_2 / ||B_k||_2 (rows of B that vanish: against the largest row)."""
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    nb = np.linalg.norm(B.astype(np.float64), axis=1)
    nb = np.where(nb > 0, nb, nb.max() if nb.max() > 0 else 1.0)
    return float((np.sqrt(np.sum((A - B) ** 2, axis=1)).astype(np.float64) / nb).max())


def energy_defect(E, Eref):
    """max over the columns of max_n |E - Eref| / max_n |Eref|."""
    E, Eref = np.asarray(E, dtype=LD), np.asarray(Eref, dtype=LD)
    return float((np.abs(E - Eref).max(axis=0) / np.abs(Eref).max(axis=0)).max())


@functools.lru_cache(maxsize=None)
def reference_defect(key, case, n_steps=200, clamped=True, source="oracle"):
    """(snapshots rel-L2, energies relative to the column maximum) of the float64 recurrence against the longdouble one: the reference's own error."""
    U64, _, _, E64 = reference_run(key, case, n_steps, clamped, np.float64, source)
    Uld, _, _, Eld = reference_run(key, case, n_steps, clamped, LD, source)
    return rel_l2_rows(U64, Uld), energy_defect(E64, Eld)


def dispersion_closed_form(phi, omega, dt, n_steps):
    """u_n = phi cos(n theta), sin(theta / 2) = omega dt / 2: central differences started from a mode shape of (K, M_L) at rest."""
    theta = 2.0 * np.arcsin(0.5 * omega * dt)
    return np.cos(theta * np.arange(n_steps + 1))[:, None] * phi[None, :]
