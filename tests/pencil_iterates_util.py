"""Reference recurrences of the two loops on the pencil A = cK K + cM M, iterate by iterate: the PCG of mfh_newmark (NewmarkWork::solve,
meshfem_amd/csrc/mfh_dynamics.hip) and the COCG of mfh_harmonic (HarmonicWork::solve, mfh_harmonic.hip) on Z = zK K + zM M. The matrices are
the oracle's pencil of tests/modes_util.py restricted to the free variables, the block-Jacobi preconditioner is harmonic_util.block_jacobi of
cK K_ff + cM M_ff, the PCG is pcg_iterates_util.pcg_classic (its scalars r.z, p.Ap, r.r are taken from the dot products it forms, in the order it
forms them) and the COCG is the recurrence of harmonic_util.cocg with the unconjugated x^T y, keeping every iterate and every scalar.

Every walk is made twice: in FP64 throughout (vectors, products and dots) and in extended precision throughout (np.longdouble / np.clongdouble,
the products summed row by row as pcg_iterates_util.csr_apply does). The extended walk is THE reference; the relative gap between the two at
iteration k is the reference's own rounding floor there, and the bound of a device iterate is tau_k = max(floor, 100 x gap_k) with floor =
TAU_ORACLE (block-Jacobi from the oracle's blocks) or TAU_HOOK (apply_M is a device hook). The factor 100 covers another summation order (two-stage
ordered sums against one long sum) and fma contraction on an ill-conditioned step. An input whose gap exceeds FLOOR_MAX is not a test input
(tests/test_pencil_iterates_reference.py asserts it for every input of tests/test_gpu_pencil_iterates.py): it is replaced, the bound is not widened.

Shared by tests/test_pencil_iterates_reference.py (CPU) and tests/test_gpu_pencil_iterates.py."""
import functools
import types

import numpy as np

import dynamics_util as D
import harmonic_util as H
import modes_util as U
import pcg_iterates_util as P

KS = (1, 2, 3, 5, 8)
KMAX = 8
TAU_ORACLE = 1e-12          # the bound of tests/test_gpu_pcg_iterates.py where apply_M comes from the oracle
TAU_HOOK = 1e-11            # ... and where it is a device hook (its launch and the loop's own are separate sums)
FLOOR_MAX = 1e-11           # the largest FP64-vs-extended gap an input of the device tests may have
KINDS = ("real", "complex")
STOP_ITERS = 12             # the walks of the stop tests: long enough for pcg_iterates_util.exact_stop on every small mesh


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def free_pencil(key):
    """(K_ff, M_ff, free, n) of the oracle's pencil clamped at modes_util.clamp_vars(key)."""
    K, M = U.pencil(key)
    free = H.free_of(key)
    return K[free][:, free].tocsr(), M[free][:, free].tocsr(), free, K.shape[0]


def expand(key, xf):
    """the full-length vector (zero on the clamp) of a vector on the free variables"""
    _, _, free, n = free_pencil(key)
    x = np.zeros(n, dtype=np.asarray(xf).dtype)
    x[free] = xf
    return x


@functools.lru_cache(maxsize=None)
def newmark_pencils(key):
    """{name: (cK, cM)} of the two solves of mfh_newmark: a trapezoidal time step at dt = T_1 / 20 (cM = 4 rho / dt^2), and the solve for the
    initial acceleration (cK = 0, cM = rho)."""
    dt = D.case_inputs(key, "undamped")["dt"]
    return {"step": (1.0, 4.0 * D.DENSITY / (dt * dt)), "accel": (0.0, D.DENSITY)}


def newmark_rhs(key):
    """(b, x0): the random load and the random start vector of dynamics_util.case_inputs, full length, zero on the clamp"""
    i = D.case_inputs(key, "undamped")
    return i["f"], i["u0"]


@functools.lru_cache(maxsize=None)
def jacobi_matrix(key, cK, cM):
    Kf, Mf, _, _ = free_pencil(key)
    return H.block_jacobi(cK * Kf + cM * Mf, U.fem_mesh(key).N)


def jacobi_apply(key, cK, cM):
    """dtype -> apply_M of the block-Jacobi of cK K_ff + cM M_ff on real vectors of that dtype (free variables)"""
    Dm = jacobi_matrix(key, cK, cM)
    return lambda dtype: P.csr_apply(Dm, dtype)


HOOK_KS = (1, 2, 3)         # the k of a walk under a K-hierarchy where its floor at k = 8 does not hold (see proxy_apply)


@functools.lru_cache(maxsize=None)
def _k_factor(key):
    return D._lu(free_pencil(key)[0])


def proxy_apply(key):
    """dtype -> r -> K_ff^-1 r by splu, in FP64 in either walk: the CPU stand-in of a K-hierarchy (two-level, multigrid) as preconditioner of the
    pencil, FP64 in and out as the device hook is. B ~ K^-1 leaves the mass-dominated low modes as outliers of B A; once their Ritz values have
    converged any two FP64 walks part exponentially, so the floor of such a walk holds for its first iterations only (HOOK_KS)."""
    lu = _k_factor(key)
    return lambda dtype: (lambda r: np.asarray(lu.solve(np.asarray(r, dtype=np.float64)), dtype=dtype))


def hook_apply(key, hook):
    """dtype -> apply_M of a device hook (full-length FP64 vectors in and out) on the free variables: the hook's FP64 map in either walk"""
    _, _, free, n = free_pencil(key)

    def make(dtype):
        def apply(r):
            full = np.zeros(n)
            full[free] = np.asarray(r, dtype=np.float64)
            return np.asarray(hook(full)[free], dtype=dtype)
        return apply
    return make


# ------------------------------------------------------------------------------------------------ the PCG on the real pencil
class _Recorder:
    """the dot product of pcg_classic, keeping every value it forms and the norms of its two arguments. pcg_classic asks for b.b, r_0.z_0 and
    then, per iteration, p.Ap, r.z and r.r"""

    def __init__(self, dot):
        self.dot, self.vals, self.scales = dot, [], []

    def __call__(self, a, b):
        v = self.dot(a, b)
        self.vals.append(v)
        self.scales.append(np.sqrt(self.dot(a, a)) * np.sqrt(self.dot(b, b)))
        return v


def _pcg_walk(A, apply_M, b, x0, iters, dtype):
    """pcg_classic from x0: the walk for b - A x0 from zero, shifted back (the loop forms r_0 = b - A x0 the same way)"""
    apply_A = P.csr_apply(A, dtype)
    nf = A.shape[0]
    x0 = np.zeros(nf, dtype=dtype) if x0 is None else np.asarray(x0, dtype=dtype)
    f = np.asarray(b, dtype=dtype) - apply_A(x0) if np.any(x0 != 0) else np.asarray(b, dtype=dtype)
    rec = _Recorder(P.dot_fp64 if dtype == np.float64 else P.dot_longdouble)
    out = P.pcg_classic(apply_A, apply_M(dtype), f, np.zeros(nf, bool), iters=iters, dot=rec, dtype=dtype)
    v, s = rec.vals, rec.scales
    assert len(v) == 2 + 3 * iters
    return types.SimpleNamespace(
        x=[np.asarray(u, dtype=np.longdouble) + x0 for u in out.u],      # (pcg_classic hands its iterates out in FP64: the floor of the gap is 1e-16)
        bb=rec.dot(np.asarray(b, dtype=dtype), np.asarray(b, dtype=dtype)),
        rz=np.array([v[1]] + [v[2 + 3 * k + 1] for k in range(iters)]), rz_scale=np.array([s[1]] + [s[2 + 3 * k + 1] for k in range(iters)]),
        pAp=np.array([v[2 + 3 * k] for k in range(iters)]), pAp_scale=np.array([s[2 + 3 * k] for k in range(iters)]),
        rr=np.array([v[0]] + [v[2 + 3 * k + 2] for k in range(iters)]))


def _gaps(w64, wx, iters, rz="rz", pp="pAp"):
    """per k = 0 .. iters: the relative gap of the iterate, and the largest scaled gap of the three scalars of that iteration"""
    gx = np.array([0.0 if not np.any(wx.x[k]) and not np.any(w64.x[k]) else rel(w64.x[k], wx.x[k]) for k in range(iters + 1)])
    gs = np.zeros(iters + 1)
    for k in range(iters + 1):
        g = [abs(getattr(w64, rz)[k] - getattr(wx, rz)[k]) / wx.rz_scale[k], abs(w64.rr[k] - wx.rr[k]) / wx.rr[k]]
        if k < iters:
            g.append(abs(getattr(w64, pp)[k] - getattr(wx, pp)[k]) / getattr(wx, pp + "_scale")[k])
        gs[k] = float(max(g))
    return gx, gs


def _finish(w64, wx, iters, floor, complex_=False):
    gx, gs = _gaps(w64, wx, iters, *(("rz", "pZp") if complex_ else ("rz", "pAp")))
    cast = np.complex128 if complex_ else np.float64
    wx.x = [np.asarray(x, dtype=cast) for x in wx.x]
    for name in ("rz", "rz_scale", "rr") + (("pZp", "pZp_scale") if complex_ else ("pAp", "pAp_scale")):
        a = getattr(wx, name)
        setattr(wx, name, np.asarray(a, dtype=cast if name in ("rz", "pZp") else np.float64))
    wx.gap_x, wx.gap_s = gx, gs
    wx.tau_x, wx.tau_s = np.maximum(floor, 100.0 * gx), np.maximum(floor, 100.0 * gs)
    wx.bb = float(wx.bb)
    wx.res = np.sqrt(wx.rr / wx.bb)          # |r_k| / |b|
    return wx


def pcg_reference(key, cK, cM, b, x0=None, apply_M=None, iters=KMAX, floor=TAU_ORACLE):
    """The extended-precision walk of the PCG on cK K_ff + cM M_ff for the full-length (b, x0): x[k] on the free variables (FP64 copies), rz[k],
    pAp[k], rr[k] with the scales |r||z|, |p||Ap|, and gap_x[k], gap_s[k], tau_x[k], tau_s[k] against the FP64 walk. apply_M: dtype -> map
    (None: the oracle's block-Jacobi)."""
    Kf, Mf, free, _ = free_pencil(key)
    A = (cK * Kf + cM * Mf).tocsr()
    apply_M = jacobi_apply(key, cK, cM) if apply_M is None else apply_M
    bf = np.asarray(b)[free]
    xf = None if x0 is None else np.asarray(x0)[free]
    walks = [_pcg_walk(A, apply_M, bf, xf, iters, dt) for dt in (np.float64, np.longdouble)]
    return _finish(walks[0], walks[1], iters, floor)


# ------------------------------------------------------------------------------------------------ the COCG on the complex pencil
def _planes(apply_M, rdtype):
    M = apply_M(rdtype)
    return lambda r: M(np.ascontiguousarray(r.real)) + 1j * M(np.ascontiguousarray(r.imag))


def cocg_walk(Kf, Mf, zK, zM, apply_M, b, x0, iters, dtype=np.complex128, rowsum=True, rtol=None, keep=True):
    """The recurrence of harmonic_util.cocg (x^T y unconjugated) from x0, every iterate and scalar kept: x[k], rz[k] = r_k^T z_k, pZp[k] = p_k^T Z p_k,
    rr[k] = the Hermitian r_k . r_k, and the scales |r||z|, |p||Z p|. dtype complex128 or clongdouble; rowsum: the products summed row by row in
    dtype (csr_apply), else scipy's (complex128 only). rtol: stop at |r_k| <= rtol |b| (k_stop; keep=False keeps the last iterate alone)."""
    rdtype = np.float64 if dtype == np.complex128 else np.longdouble
    if rowsum:
        aK, aM = P.csr_apply(Kf, dtype), P.csr_apply(Mf, dtype)
    else:
        assert dtype == np.complex128
        aK, aM = (lambda v: Kf @ v), (lambda v: Mf @ v)
    zK, zM = dtype(zK), dtype(zM)
    haveK = zK != 0

    def Z(v):
        return zK * aK(v) + zM * aM(v) if haveK else zM * aM(v)
    B = _planes(apply_M, rdtype)
    norm = lambda v: np.sqrt(np.sum(v.real * v.real + v.imag * v.imag))
    b = np.asarray(b, dtype=dtype)
    x = np.zeros(len(b), dtype=dtype) if x0 is None else np.asarray(x0, dtype=dtype).copy()
    r = b - Z(x) if np.any(x != 0) else b.copy()
    z = B(r)
    p = z.copy()
    rho = np.dot(r, z)
    w = types.SimpleNamespace(x=[x.copy()], rz=[rho], rz_scale=[norm(r) * norm(z)], pZp=[], pZp_scale=[], rr=[norm(r) ** 2], k_stop=None)
    bb = w.bb = norm(b) ** 2
    for k in range(iters):
        if rtol is not None and w.rr[-1] <= rtol * rtol * bb:
            w.k_stop = k
            break
        q = Z(p)
        mu = np.dot(p, q)
        alpha = rho / mu
        x = x + alpha * p
        r = r - alpha * q
        z = B(r)
        rho_new = np.dot(r, z)
        w.pZp.append(mu)
        w.pZp_scale.append(norm(p) * norm(q))
        p = z + (rho_new / rho) * p
        rho = rho_new
        if keep:
            w.x.append(x.copy())
        else:
            w.x = [x.copy()]
        w.rz.append(rho)
        w.rz_scale.append(norm(r) * norm(z))
        w.rr.append(norm(r) ** 2)
    for name in ("rz", "rz_scale", "pZp", "pZp_scale", "rr"):
        setattr(w, name, np.array(getattr(w, name)))
    return w


def cocg_reference(key, zK, zM, jacobi_cM, f, x0=None, apply_M=None, iters=KMAX, floor=TAU_ORACLE):
    """The extended-precision walk of the COCG on zK K_ff + zM M_ff for the full-length (f, x0), as pcg_reference: x[k] (complex128 copies), rz[k],
    pZp[k] complex, rr[k], the scales, the gaps against the complex128 walk and the bounds. apply_M: dtype -> the real map applied to each plane
    (None: the oracle's block-Jacobi of K + jacobi_cM M)."""
    Kf, Mf, free, _ = free_pencil(key)
    apply_M = jacobi_apply(key, 1.0, jacobi_cM) if apply_M is None else apply_M
    ff = np.asarray(f)[free]
    xf = None if x0 is None else np.asarray(x0)[free]
    walks = [cocg_walk(Kf, Mf, zK, zM, apply_M, ff, xf, iters, dt) for dt in (np.complex128, np.clongdouble)]
    return _finish(walks[0], walks[1], iters, floor, complex_=True)


def harmonic_inputs(key, case, w):
    """(zK, zM, jacobi cM) of mfh_harmonic at the frequency w: harmonic_util.coefficients and the blocks of K + w^2 rho M"""
    zK, zM = H.coefficients(key, case, float(w))
    return zK, zM, float(w) * float(w) * H.DENSITY


def stop_harmonic(key):
    """(case, frequency) of the stop tests of the COCG: Rayleigh damping at omega_1 / 2"""
    return "rayleigh", H.sweep_omegas(key)[1]


def stop_rule(res):
    """(k*, rtol) of pcg_iterates_util.exact_stop on the residual history |r_k| / |b|"""
    return P.exact_stop(list(res))
