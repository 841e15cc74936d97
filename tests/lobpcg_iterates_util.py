"""Reference recurrence of the block LOBPCG loop that mfh_modes, mfh_modes_many, mfh_buckling and mfh_modes_prestressed share (lobpcg_run /
struct Lobpcg, meshfem_amd/csrc/mfh_modes.hip), iterate by iterate, written from docs/design/04_12_modes.md ("The iteration") on dense blocks of
the free variables:

  start      S0 restricted to the free variables, Z projected out, Q projected out twice, B-orthonormalised, Rayleigh-Ritz on it
  per k      R = A X - B X diag(lam); with a deflation set R -= BQ (Q^T R); res_j = |R_j| / (|lam_j| |B X_j|); a column with res_j <= rtol is locked
             W = T R on the columns that are not locked, W -= Z (BZ)^T W, W -= Q (BQ)^T W
             the basis [X, W_act, P_act] B-orthonormalised in that order (a scaled pivot <= 1e-12 in P drops P -- a restart --, in W that column and P)
             Rayleigh-Ritz on the basis: X+ = S C, P+ = [W P] C' (the W and P rows of C), lam = the m smallest Ritz values

The pencils (A, B): vibration (K, rho M) from modes_util.pencil; buckling (Kg, K) from buckling_util.stiffness / Kg_of; prestressed
(K + s Kg, rho M) with prestress_util.mass. T is the block-Jacobi of K (pcg_iterates_util.block_jacobi_blocks, the FP64 inverse blocks applied in
the walk's precision) or a device hook (pencil_iterates_util.hook_apply).

Every walk is made twice: in FP64 throughout and in extended precision (np.longdouble) throughout -- the sparse products summed row by row, the
Gram matrices, the Cholesky factors of the orthonormalisation and the small eigenproblem (cyclic Jacobi in np.longdouble, started from the FP64
eigenvectors). The extended walk is THE reference; the gap between the two at iteration k, in the very measures the device is held to, is the
reference's own floor, and the bound of a device quantity is tau_k = max(floor, 100 x gap_k) with pencil_iterates_util's TAU_ORACLE / TAU_HOOK and
its reasoning for the factor 100. An input whose gap exceeds FLOOR_MAX at a k it is walked to is replaced, the bound is not widened
(tests/test_lobpcg_iterates_reference.py asserts it for every input of tests/test_gpu_lobpcg_iterates.py).

What is compared is invariant under the choice of an orthonormal basis, so nothing here imitates Cholesky-QR's columns: all m Ritz values (error
relative to max |lam| of the block: buckling and prestressed values change sign), all m relative residuals (relatively), and subspaces -- the
reference's Ritz values at k are clustered (neighbours closer than CLUSTER x the spread of the block belong together), and per cluster c
|(I - X_c,ref X_c,ref^T B) X_c,dev|_B / |X_c,dev|_B; the same for the whole block.

Shared by tests/test_lobpcg_iterates_reference.py (CPU) and tests/test_gpu_lobpcg_iterates.py."""
import collections
import functools
import types

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import buckling_util as B
import modes_util as U
import pcg_iterates_util as P
import pencil_iterates_util as R
import prestress_util as PS

KS = R.KS
KMAX = R.KMAX
HOOK_KS = R.HOOK_KS
TAU_ORACLE, TAU_HOOK, FLOOR_MAX = R.TAU_ORACLE, R.TAU_HOOK, R.FLOOR_MAX
BLK_MAXC = 24
DROP = 1e-12                # the loop's rule: a scaled Cholesky pivot at or below it drops the column
PIVOT_MIN = 1e-8            # what every walked input keeps its pivots above: four decades clear of the rule, so no rank decision is in doubt
# Neighbouring Ritz values of the reference closer than CLUSTER x (max lam - min lam of the block) are compared as one subspace. A reference-only
# choice: an invariant subspace moves by eps / gap under rounding, so the threshold is what keeps the subspace floors of every input below FLOOR_MAX.
# Measured on the CPU (tests/test_lobpcg_iterates_reference.py prints them; docs/design/04_12_modes.md, "Iterates pinned", has the table).
CLUSTER = 1e-3
XD = np.longdouble

Case = collections.namedtuple("Case", "pencil key nev seed density ratio free nq ks rtol smooth field")


def _case(pencil, key, nev, seed=11, density=1.0, ratio=0.0, free=False, nq=0, ks=KS, rtol=0.0, smooth=0, field="axial"):
    return Case(pencil, key, nev, seed, density, ratio, free, nq, tuple(ks), rtol, smooth, field)


def case_name(c):
    key = "%dD-P%d" % c.key if isinstance(c.key, tuple) else c.key
    extra = "".join([" rho%g" % c.density if c.density != 1.0 else "", " s%g" % c.ratio if c.pencil == "prestressed" else "", " free" if c.free else "",
                     " nq%d" % c.nq if c.nq else "", " " + c.field if c.field != "axial" else "", " rtol%.3g" % c.rtol if c.rtol else ""])
    return "%s %s nev%d%s" % (c.pencil, key, c.nev, extra)


# ------------------------------------------------------------------------------------------------ the inputs of the device tests
CLAMPED = [_case("vibration", key, nev) for key in U.SMALL for nev in (1, 4)]
DENSITY = [_case("vibration", (2, 2), 4, density=2.7)]
FREE_BODY = [_case("vibration", key, 4, free=True) for key in ((2, 2), (3, 1))]
FULL_BLOCK = [_case("vibration", (3, 2), 20, ks=(1, 2, 3))]
COLUMN_KEYS = ("col3d-P1", "strip-P2")
# under axial compression Kg is negative semidefinite and every mu is negative; the random symmetric prestress field puts both signs into the
# Rayleigh-Ritz of the start block (later blocks hold the m smallest values, all negative)
BUCKLING = [_case("buckling", key, 3, field=f) for key in COLUMN_KEYS for f in ("axial", "random")]
PRESTRESSED = [_case("prestressed", key, 3, ratio=r) for key in COLUMN_KEYS for r in (0.5, 1.1)]
DEFLATED = [_case("vibration", key, 4, nq=7) for key in ((3, 1), (2, 2))]
WALKED = CLAMPED + DENSITY + FREE_BODY + FULL_BLOCK + BUCKLING + PRESTRESSED + DEFLATED
STOP_ITERS = 12             # the longest walk of a stop case
STOP_RTOLS = tuple(float("%.2e" % r) for r in np.geomspace(1e-3, 0.6, 20))          # the thresholds find_stop chooses from
STOP = [_case("vibration", (2, 2), 4, smooth=(3e-5, 1e-2)), _case("vibration", (3, 2), 4, smooth=(1.2e-5, 1e-3))]          # (rtol comes from find_stop)


def block_size(nev, n_eff):
    return min(nev + max(2, (nev + 3) // 4), BLK_MAXC, n_eff)


# ------------------------------------------------------------------------------------------------ the pencil of a case
def prestress(case):
    """the prestress field of a buckling or prestressed case: unit axial compression, or buckling_util.random_symmetric_field"""
    if case.field == "axial":
        return B.axial_compression(case.key)
    en, pos = B.mesh_tables(case.key)
    return B.random_symmetric_field(len(en), pos.shape[1], 3)


@functools.lru_cache(maxsize=None)
def problem(case):
    """The matrices of a case on the free variables and its start block: A, B (CSR), K (CSR, for T), Kfull and the fixed mask (for the blocks),
    Z [nf, nz] or None (the rigid modes as modes_util builds them), Q [nf, nq] or None (B-orthonormalised on the host), S0 [m, n] (seeded normal
    values, non-zero on the fixed rows), free, n, bs, m."""
    key = case.key
    if case.pencil == "vibration":
        K, Mm = U.pencil(key)
        bs = U.fem_mesh(key).N
        fixed = np.zeros(0, dtype=np.int64) if case.free else U.clamp_vars(key)
        Afull, Bfull = K, case.density * Mm
        pos = np.asarray(U.fem_mesh(key).node_pos)
    else:
        K = B.stiffness(key)
        bs = B.fem_mesh(key).N
        fixed = B.clamp_vars(key)
        G = sp.csr_matrix(B.Kg_of(key, prestress(case)))
        if case.pencil == "buckling":
            Afull, Bfull = G, K
        else:
            Afull, Bfull = K + (case.ratio * PS.critical_factor(key)) * G, case.density * PS.mass(key)
        pos = None
    n = K.shape[0]
    mask = np.zeros(n, bool)
    mask[fixed] = True
    free = np.nonzero(~mask)[0]
    cut = lambda Mx: sp.csr_matrix(Mx)[free][:, free].tocsr()
    Af, Bf, Kf = cut(Afull), cut(Bfull), cut(K)
    Z = U.rigid_modes(pos)[free] if case.free else None
    nz = 0 if Z is None else Z.shape[1]
    rng = np.random.default_rng(case.seed)
    Q = None
    if case.nq:
        Q = U.m_orthonormalise(np.random.default_rng(case.seed + 1000).standard_normal((len(free), case.nq)), Bf)
    m = block_size(case.nev, len(free) - nz - case.nq)
    S0 = rng.standard_normal((m, n))
    if case.smooth:
        # The stop cases. Under block-Jacobi the residuals of a random block fall by a fifth per iteration, so a column spends several iterations
        # within a factor 2 of any threshold. This start makes them jump, as pcg_iterates_util.two_eigenvector_rhs does for the PCG: column j < nev
        # is the eigenvector v_j plus 1e-3 of u, a top eigenvector of A u = theta D u (D the block-Jacobi blocks). T (A - lam_j B) u = theta u up
        # to lam_j T B u << theta u, so W_j is u almost alone and span[x_j, W_j] holds v_j: the residual falls by orders of magnitude in ONE
        # iteration. The last of the nev columns carries two such directions and needs P and a second iteration; the guard columns stay random.
        assert case.pencil == "vibration" and not case.free
        unit = lambda v: v / np.linalg.norm(v, axis=0) * np.sign(v[np.abs(v).argmax(axis=0), np.arange(v.shape[1])])
        v0 = np.ones(len(free))
        lv, V = spla.eigsh(Af.tocsc(), k=m, M=Bf.tocsc(), sigma=0.0, which="LM", v0=v0, tol=1e-12)
        V = unit(V[:, np.argsort(lv)])
        Dff = cut(sp.block_diag(list(P.block_jacobi_blocks(K, bs, mask)), format="csr"))
        th, Uh = spla.eigsh(Af.tocsc(), k=case.nev, M=Dff.tocsc(), which="LA", v0=v0, tol=1e-12)
        Uh = unit(Uh[:, np.argsort(th)])
        Um = unit(spla.eigsh(Af.tocsc(), k=1, M=Dff.tocsc(), sigma=th.max() / 5.0, which="LM", v0=v0, tol=1e-12)[1])
        Sf = S0[:, free].T / np.sqrt(len(free))
        for j in range(case.nev - 1):
            Sf[:, j] = V[:, j] + case.smooth[0] * Uh[:, j]
        Sf[:, case.nev - 1] = V[:, case.nev - 1] + case.smooth[1] * (Uh[:, case.nev - 1] + Um[:, 0])
        S0[:, free] = Sf.T
    Binv = np.linalg.inv(P.block_jacobi_blocks(K, bs, mask))
    for a in (S0, free, Binv) + (() if Q is None else (Q,)):
        a.setflags(write=False)
    return types.SimpleNamespace(A=Af, B=Bf, K=Kf, Binv=Binv, mask=mask, Z=Z, Q=Q, S0=S0, free=free, n=n, bs=bs, m=m, nf=len(free))


def expand(p, Xf):
    """[cols, n] rows of full-length vectors (zero on the fixed variables) from a block [nf, cols] on the free variables"""
    X = np.zeros((Xf.shape[1], p.n))
    X[:, p.free] = np.asarray(Xf, dtype=np.float64).T
    return X


def jacobi_T(p):
    """dtype -> W = T R on blocks of the free variables: the FP64 inverse diagonal blocks of K (the fixed components decoupled), applied in dtype"""
    def make(dtype):
        Binv = p.Binv.astype(dtype)

        def apply(Rf):
            full = np.zeros((p.n, Rf.shape[1]), dtype=dtype)
            full[p.free] = Rf
            z = np.einsum("qab,qbc->qac", Binv, full.reshape(-1, p.bs, Rf.shape[1])).reshape(p.n, -1)
            return z[p.free]
        return apply
    return make


def hook_T(p, hook):
    """dtype -> the same from a device hook on full-length FP64 vectors (the hook's FP64 map in either walk)"""
    def make(dtype):
        def apply(Rf):
            out = np.empty(Rf.shape, dtype=dtype)
            for j in range(Rf.shape[1]):
                full = np.zeros(p.n)
                full[p.free] = np.asarray(Rf[:, j], dtype=np.float64)
                out[:, j] = hook(full)[p.free]
            return out
        return apply
    return make


# ------------------------------------------------------------------------------------------------ dense pieces in either precision
def _spmm(Mx, dtype):
    Mx = sp.csr_matrix(Mx)
    if dtype == np.float64:
        return lambda V: Mx @ V
    Mx.sort_indices()
    data, idx, starts = Mx.data.astype(dtype)[:, None], Mx.indices, Mx.indptr[:-1]
    assert np.all(np.diff(Mx.indptr) > 0), "an empty row"

    def apply(V):
        V = np.asarray(V, dtype=dtype)
        out = np.empty((len(starts), V.shape[1]), dtype=dtype)
        for c0 in range(0, V.shape[1], 8):          # (eight columns at a time: the products of a chunk are held at once)
            out[:, c0:c0 + 8] = np.add.reduceat(data * V[idx, c0:c0 + 8], starts, axis=0)
        return out
    return apply


def _scaled_cholesky(G):
    """(index of the first scaled pivot <= DROP or -1, the pivots seen, U with U^T G U = I): Cholesky of D^-1/2 G D^-1/2 in G's precision"""
    k = len(G)
    G = (G + G.T) / 2
    d = np.sqrt(np.diag(G))
    Gs = G / np.outer(d, d)
    L = np.zeros_like(G)
    piv = np.full(k, np.nan)
    for j in range(k):
        v = Gs[j:, j] - L[j:, :j] @ L[j, :j]
        piv[j] = float(v[0])
        if not v[0] > DROP:
            return j, piv, None
        L[j:, j] = v / np.sqrt(v[0])
    Linv = np.zeros_like(G)
    for i in range(k):
        e = np.zeros(k, dtype=G.dtype)
        e[i] = 1
        Linv[i] = (e - L[i, :i] @ Linv[:i]) / L[i, i]
    return -1, piv, Linv.T / d[:, None]


def _sym_eig(G, dtype):
    """(w ascending, V) of a symmetric matrix: numpy's eigh in FP64; in extended precision cyclic Jacobi on V64^T G V64"""
    G = (G + G.T) / 2
    w, V = np.linalg.eigh(np.asarray(G, dtype=np.float64))
    if dtype == np.float64:
        return w, V
    V = V.astype(dtype)
    C = V.T @ G @ V
    C = (C + C.T) / 2
    k = len(C)
    scale = np.abs(np.diag(C)).max()
    for sweep in range(20):
        turned = 0
        for a in range(k - 1):
            for b in range(a + 1, k):
                if abs(C[a, b]) <= 1e-24 * scale:
                    continue
                turned += 1
                theta = (C[b, b] - C[a, a]) / (2 * C[a, b])
                t = (1 if theta >= 0 else -1) / (abs(theta) + np.sqrt(theta * theta + 1))
                cs = 1 / np.sqrt(t * t + 1)
                sn = t * cs
                for Mx in (C, V):
                    ca, cb = Mx[:, a].copy(), Mx[:, b].copy()
                    Mx[:, a], Mx[:, b] = cs * ca - sn * cb, sn * ca + cs * cb
                ra, rb = C[a].copy(), C[b].copy()
                C[a], C[b] = cs * ra - sn * rb, sn * ra + cs * rb
        if not turned:
            break
    else:
        raise AssertionError("the extended-precision Jacobi did not settle")
    w = np.diag(C).copy()
    order = np.argsort(w, kind="stable")
    return w[order], V[:, order]


# ------------------------------------------------------------------------------------------------ the walk
def walk(p, make_T, nev, iters, dtype, rtol=0.0, keep=True):
    """The recurrence of the module docstring in one precision. Per call k = 0 .. of the convergence check: lam[k], res[k] (all m columns), X[k]
    [nf, m], sets[k] = (|W|, |P|, restarts) of the iteration before, pivots[k] = the smallest scaled pivot of that iteration's basis (first pass).
    Stops where the first nev columns pass rtol (k_stop) or after iters iterations."""
    aA, aB, T = _spmm(p.A, dtype), _spmm(p.B, dtype), make_T(dtype)
    m = p.m
    col_norm = lambda V: np.sqrt(np.sum(V * V, axis=0))
    Z = BZ = Q = BQ = None
    if p.Z is not None:
        Z = np.asarray(p.Z, dtype=dtype)
        for _ in range(2):
            Z = Z @ _scaled_cholesky(Z.T @ aB(Z))[2]
        BZ = aB(Z)
    if p.Q is not None:
        Q = np.asarray(p.Q, dtype=dtype)
        BQ = aB(Q)
    X = np.asarray(p.S0, dtype=dtype).T[p.free]
    if Z is not None:
        X = X - Z @ (BZ.T @ X)
    if Q is not None:
        for _ in range(2):
            X = X - Q @ (BQ.T @ X)
    piv0 = np.inf
    for ps in range(2):
        bad, piv, Um = _scaled_cholesky(X.T @ aB(X))
        assert bad < 0, "the start block is rank deficient"
        piv0 = min(piv0, piv.min()) if ps == 0 else piv0
        X = X @ Um
    lam, C = _sym_eig(X.T @ aA(X), dtype)
    X = X @ C
    Pb = np.zeros_like(X)
    haveP = False
    restarts = 0
    out = types.SimpleNamespace(lam=[], res=[], X=[], sets=[(0, 0, 0)], pivots=[float(piv0)], k_stop=None, m=m)
    for k in range(iters + 1):
        AX, BX = aA(X), aB(X)
        Rm = AX - BX * lam[None, :]
        if Q is not None:
            Rm = Rm - BQ @ (Q.T @ Rm)
        res = col_norm(Rm) / (np.abs(lam) * col_norm(BX))
        out.lam.append(lam.copy())
        out.res.append(res.copy())
        if keep:
            out.X.append(X.copy())
        else:
            out.X = [X.copy()]
        conv = res <= rtol
        if np.all(conv[:nev]):
            out.k_stop = k
            break
        if k == iters:
            break
        act = np.nonzero(~conv)[0]
        W = T(Rm[:, act])
        if Z is not None:
            W = W - Z @ (BZ.T @ W)
        if Q is not None:
            W = W - Q @ (BQ.T @ W)
        Pa = Pb[:, act] if haveP else Pb[:, :0]
        pmin = np.inf
        for ps in range(2):
            while True:
                S = np.concatenate([X, W, Pa], axis=1)
                bad, piv, Um = _scaled_cholesky(S.T @ aB(S))
                if ps == 0:
                    pmin = min(pmin, np.nanmin(piv))
                if bad >= m + W.shape[1]:
                    Pa, haveP, restarts = Pa[:, :0], False, restarts + 1
                elif bad >= m:
                    W = np.delete(W, bad - m, axis=1)
                    if Pa.shape[1]:
                        Pa, haveP, restarts = Pa[:, :0], False, restarts + 1
                elif bad >= 0:
                    raise AssertionError("the Ritz block lost its rank")
                else:
                    break
            S = S @ Um
            X, W, Pa = S[:, :m], S[:, m:m + W.shape[1]], S[:, m + W.shape[1]:]
        nw, npc = W.shape[1], Pa.shape[1]
        S = np.concatenate([X, W, Pa], axis=1)
        ev, C = _sym_eig(S.T @ aA(S), dtype)
        X = S @ C[:, :m]
        Pb = S[:, m:] @ C[m:, :m]
        lam = ev[:m]
        haveP = nw > 0
        out.sets.append((nw, npc, restarts))
        out.pivots.append(float(pmin))
    return out


def _b_norm2(aB, V):
    return float(np.sum(V * aB(V)))


def clusters(lam):
    """index lists: consecutive values of lam (ascending) closer than CLUSTER x the block's spread belong together"""
    lam = np.asarray(lam, dtype=np.float64)
    spread = max(lam.max() - lam.min(), np.abs(lam).max() * 1e-300)
    out, cur = [], [0]
    for j in range(1, len(lam)):
        if lam[j] - lam[j - 1] < CLUSTER * spread:
            cur.append(j)
        else:
            out.append(cur)
            cur = [j]
    out.append(cur)
    return out


def measures(p, ref, k, lam, res, Xf):
    """The three errors of (lam, res, X [nf, m] or None) against iterate k of the extended walk ref: (max |lam - lam_ref| / max |lam_ref|,
    max |res - res_ref| / res_ref, the largest subspace defect over the clusters of lam_ref and the whole block)."""
    lr, rr = ref.lam[k], ref.res[k]
    e_lam = float(np.abs(np.asarray(lam, dtype=XD) - lr).max() / np.abs(lr).max())
    e_res = float((np.abs(np.asarray(res, dtype=XD) - rr) / rr).max())
    e_sub = 0.0
    if Xf is not None:
        aB = _spmm(p.B, XD)
        Xr, Xd = ref.X[k], np.asarray(Xf, dtype=XD)
        BXr = aB(Xr)
        for c in clusters(lr) + [list(range(len(lr)))]:
            D = Xd[:, c] - Xr[:, c] @ (BXr[:, c].T @ Xd[:, c])
            e_sub = max(e_sub, float(np.sqrt(_b_norm2(aB, D) / _b_norm2(aB, Xd[:, c]))))
    return e_lam, e_res, e_sub


def reference(case, make_T=None, iters=None, floor=TAU_ORACLE):
    """The extended walk of a case (X[k] longdouble on the free variables) with, per k, gap_* = measures() of the FP64 walk against it and tau_* =
    max(floor, 100 gap): .gap_lam, .gap_res, .gap_sub, .tau_lam, .tau_res, .tau_sub; .sets64 / .k_stop64 the FP64 walk's own sets and stop."""
    p = problem(case)
    make_T = jacobi_T(p) if make_T is None else make_T
    iters = max(case.ks) if iters is None else iters
    w64 = walk(p, make_T, case.nev, iters, np.float64, case.rtol)
    ref = walk(p, make_T, case.nev, iters, XD, case.rtol)
    nk = min(len(ref.lam), len(w64.lam))
    g = np.array([measures(p, ref, k, w64.lam[k], w64.res[k], w64.X[k]) for k in range(nk)])
    ref.gap_lam, ref.gap_res, ref.gap_sub = g[:, 0], g[:, 1], g[:, 2]
    ref.tau_lam, ref.tau_res, ref.tau_sub = (np.maximum(floor, 100.0 * g[:, j]) for j in range(3))
    ref.sets64, ref.k_stop64 = w64.sets, w64.k_stop
    ref.restarts = ref.sets[-1][2]
    return ref


@functools.lru_cache(maxsize=None)
def jacobi_reference(case, iters=None):
    """reference() under the oracle's block-Jacobi, once per process"""
    return reference(case, None, iters, TAU_ORACLE)


def monotone_defect(lam_hist, tau):
    """the largest rise of a Ritz value from one check to the next, relative to max |lam| of the block there, minus nothing: <= tau is monotone
    (Cauchy interlacing: X_k lies in the basis of iteration k + 1, so lam_j cannot rise)"""
    lam_hist = np.asarray(lam_hist, dtype=np.float64)
    if len(lam_hist) < 2:
        return 0.0
    rise = (lam_hist[1:] - lam_hist[:-1]) / np.abs(lam_hist[:-1]).max(axis=1)[:, None]
    return float(max(rise.max(), 0.0))


# ------------------------------------------------------------------------------------------------ the stop and the soft lock
def stop_margin(ref, rtol):
    """(k*, the number of columns locked before k*, the smallest factor between rtol and a reference residual at k <= k*)"""
    res = np.array([np.asarray(r, dtype=np.float64) for r in ref.res])
    ks = ref.k_stop
    assert ks is not None, "the walk did not stop"
    locked_before = int((res[:ks] <= rtol).any(axis=0).sum()) if ks > 0 else 0
    ratio = np.maximum(res[:ks + 1] / rtol, rtol / res[:ks + 1])
    return ks, locked_before, float(ratio.min())


def find_stop(case, make_T=None, floor=TAU_ORACLE):
    """(rtol, reference walk under it) of a stop case, from the residual histories of the recurrence itself: of the thresholds
    STOP_RTOLS the one under which the FP64 walk WITH the lock stops latest (then: with the widest margin) while a column locks before the
    stop and no residual of any column up to the stop lies within a factor 2 of the threshold -- so that rounding cannot move the stop or a
    lock to a neighbouring iteration. The extended walk under that threshold is then held to the same conditions."""
    p = problem(case)
    T = jacobi_T(p) if make_T is None else make_T
    best = None
    for rtol in STOP_RTOLS:
        w = walk(p, T, case.nev, STOP_ITERS, np.float64, rtol)
        if w.k_stop is None or w.k_stop < 1:
            continue
        k_stop, locked_before, margin = stop_margin(w, rtol)
        if locked_before >= 1 and margin >= 2.2 and (best is None or (k_stop, margin) > best[:2]):
            best = (k_stop, margin, rtol)
    assert best is not None, "no threshold with a factor-2 margin and an earlier lock: another start block or nev"
    rtol = best[2]
    ref = reference(case._replace(rtol=rtol), T, STOP_ITERS, floor)
    k_stop, locked_before, margin = stop_margin(ref, rtol)
    assert ref.k_stop64 == k_stop and locked_before >= 1 and margin >= 2.0, (k_stop, ref.k_stop64, locked_before, margin)
    return rtol, ref


@functools.lru_cache(maxsize=None)
def jacobi_stop(case):
    return find_stop(case)
