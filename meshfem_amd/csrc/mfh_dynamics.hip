// Transient dynamics (mfh_newmark, include/meshfem_hip.h; docs/design/04_13_dynamics.md): implicit Newmark time stepping of
//   M u'' + C u' + K u = g(t) f,   M = density x the consistent vector mass matrix,  C = aR M + bR K,  fixed variables held at zero.
// The reference has no time integrator; the scheme is checked against an independent recurrence (tests/dynamics_util.py). Every step solves
//   A u+ = b,   A = cK K + cM M  (the "pencil operator"),   cK = 1 + gamma bR / (beta dt),  cM = density (1 / (beta dt^2) + gamma aR / (beta dt))
// by a PCG loop of this file on the context's operator (apply_operator) and preconditioners (launch of k_pencil_dinv's blocks / tl_precond /
// mg_precond), the way mfh_modes.hip builds on them without touching the pinned loops of mfh_solver.cpp.
//   k_newmark_predict  u~, v~, the vector M multiplies and the vector K multiplies, one pass over (u, v, a)
//   k_newmark_rhs      b = g f + (products), masked, with b . b
//   k_newmark_correct  a+, v+, u+, the probe values of the step and the snapshot row
//   k_dyn_*            the PCG's vector kernels
#include "mfh_pencil.hh"      // shared with mfh_harmonic.hip: the gate, the ordered sums, k_spmv_kron_acc, k_pencil_dinv, and the loop's setup and host driver

namespace mfh { namespace k {

namespace {

// ---- the step kernels
struct PredictArgs {
    int64_t n;
    double dt, cua, cva;       // u~ = u + dt v + cua a,  v~ = v + cva a
    double cw;                 // w = cw u~ - v~  (the vector C multiplies; cw = gamma / (beta dt))
    double cmu, cmw, ckw;      // xm = cmu u~ + cmw w (density inside),  xk = ckw w
};
__global__ void __launch_bounds__(256) k_newmark_predict(PredictArgs p, const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ a,
                                                        const uint8_t *__restrict__ mask, double *__restrict__ ut, double *__restrict__ vt,
                                                        double *__restrict__ xm, double *__restrict__ xk) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * 256) {
        const double ai = a[i], vi = v[i];
        double up = fma(p.cua, ai, fma(p.dt, vi, u[i])), vp = fma(p.cva, ai, vi);
        if (mask && mask[i]) { up = 0.0; vp = 0.0; }
        const double w = fma(p.cw, up, -vp);
        ut[i] = up;
        vt[i] = vp;
        xm[i] = fma(p.cmu, up, p.cmw * w);
        if (xk) xk[i] = p.ckw * w;
    }
}

// b = g f + y (f null: y alone), zero on the fixed variables; partials[.][0] = b . b
__global__ void __launch_bounds__(256) k_newmark_rhs(int64_t n, double g, const double *__restrict__ f, const double *__restrict__ y,
                                                    const uint8_t *__restrict__ mask, double *__restrict__ b, double *__restrict__ partials) {
    __shared__ double red[8];
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double v = f ? fma(g, f[i], y[i]) : y[i];
        if (mask && mask[i]) v = 0.0;
        b[i] = v;
        acc[0] = fma(v, v, acc[0]);
    }
    store_partials<1>(acc, red, partials);
}

struct CorrectArgs {
    int64_t n;
    double ca, cv;             // a+ = ca (x - u~),  v+ = v~ + cv a+   (ca = 1 / (beta dt^2), cv = gamma dt)
    int recordOnly;            // 1: u, v, a stay; the probe values and the snapshot row are taken from u (step 0)
    int nProbe;
    const int64_t *probeVars;
    double *probeRow;          // nProbe values of this step (null: no probes)
    double *snapRow;           // n values (null: not a snapshot step)
};
__global__ void __launch_bounds__(256) k_newmark_correct(CorrectArgs p, const double *__restrict__ x, const double *__restrict__ ut, const double *__restrict__ vt,
                                                        double *__restrict__ u, double *__restrict__ v, double *__restrict__ a) {
    const double *src = p.recordOnly ? u : x;
    // the probes read the solution itself, which no lane of this kernel writes (x) or which stays as it is (u, recordOnly)
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < p.nProbe; j += (int64_t)gridDim.x * 256) p.probeRow[j] = src[p.probeVars[j]];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * 256) {
        const double xi = src[i];
        if (p.snapRow) p.snapRow[i] = xi;
        if (!p.recordOnly) {
            const double an = p.ca * (xi - ut[i]);
            a[i] = an;
            v[i] = fma(p.cv, an, vt[i]);
            u[i] = xi;
        }
    }
}

// partials[.][0] = a . b, [.][1] = c . a (c null: 0)
__global__ void __launch_bounds__(256) k_dyn_dot2(int64_t n, const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ c,
                                                 double *__restrict__ partials) {
    __shared__ double red[8];
    double acc[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double ai = a[i];
        acc[0] = fma(ai, b[i], acc[0]);
        if (c) acc[1] = fma(c[i], ai, acc[1]);
    }
    store_partials<2>(acc, red, partials);
}

// ---- the PCG's vector kernels (one lane per block row: DIM consecutive variables)
// r = b - Ax; BJ: z = Dinv r, p = z, partials {r.z, r.r}; else partials {-, r.r}. bb == 0 (a zero right-hand side): x = 0 is the solution (the rule of
// mfh_solve), r = z = p = 0.
template <int DIM, bool BJ>
__global__ void __launch_bounds__(256) k_dyn_init(int64_t nRows, const double *__restrict__ dinv, const double *__restrict__ b, const double *__restrict__ Ax,
                                                 const double *__restrict__ bb, double *__restrict__ x, double *__restrict__ r, double *__restrict__ z,
                                                 double *__restrict__ p, double *__restrict__ partials) {
    __shared__ double red[8];
    constexpr int NS = DIM * (DIM + 1) / 2;
    const bool zeroRhs = bb[0] == 0.0;
    double acc[2] = {0.0, 0.0};
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < nRows; n += (int64_t)gridDim.x * 256) {
        double rv[DIM], zv[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) rv[c] = zeroRhs ? 0.0 : b[n * DIM + c] - Ax[n * DIM + c];
        if (BJ) apply_packed<DIM>(dinv + n * NS, rv, zv);
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            r[n * DIM + c] = rv[c];
            if (zeroRhs) x[n * DIM + c] = 0.0;
            if (BJ) { z[n * DIM + c] = zv[c]; p[n * DIM + c] = zv[c]; acc[0] = fma(rv[c], zv[c], acc[0]); }
            acc[1] = fma(rv[c], rv[c], acc[1]);
        }
    }
    store_partials<2>(acc, red, partials);
}

// alpha = r.z / p.Ap of iteration it;  x += alpha p;  r -= alpha Ap;  BJ: z = Dinv r, partials {r.z, r.r}; else {-, r.r}
template <int DIM, bool BJ>
__global__ void __launch_bounds__(256) k_dyn_update(int64_t nRows, const double *__restrict__ dinv, const double *__restrict__ Ap, const double *__restrict__ p,
                                                   double *__restrict__ x, double *__restrict__ r, double *__restrict__ z, DynGate g,
                                                   double *__restrict__ partials) {
    __shared__ double red[8];
    constexpr int NS = DIM * (DIM + 1) / 2;
    if (dyn_closed(g)) return;
    const double *sc = g.scal + (int64_t)(g.it + (int)g.stop[3]) * 4;
    const double alpha = sc[0] / sc[1];
    double acc[2] = {0.0, 0.0};
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < nRows; n += (int64_t)gridDim.x * 256) {
        double rv[DIM], zv[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            const int64_t i = n * DIM + c;
            x[i] = fma(alpha, p[i], x[i]);
            rv[c] = fma(-alpha, Ap[i], r[i]);
            r[i] = rv[c];
            acc[1] = fma(rv[c], rv[c], acc[1]);
        }
        if (BJ) {
            apply_packed<DIM>(dinv + n * NS, rv, zv);
#pragma unroll
            for (int c = 0; c < DIM; ++c) { z[n * DIM + c] = zv[c]; acc[0] = fma(rv[c], zv[c], acc[0]); }
        }
    }
    store_partials<2>(acc, red, partials);
}

// after the two-level / multigrid preconditioner: z = r on the fixed variables (r is 0 there), partials {r.z}
__global__ void __launch_bounds__(256) k_dyn_rz(int64_t n, const double *__restrict__ r, double *__restrict__ z, const uint8_t *__restrict__ mask, DynGate g,
                                               double *__restrict__ partials) {
    __shared__ double red[8];
    if (dyn_closed(g)) return;
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double zv = z[i];
        const double rv = r[i];
        if (mask && mask[i]) { zv = rv; z[i] = zv; }
        acc[0] = fma(rv, zv, acc[0]);
    }
    store_partials<1>(acc, red, partials);
}

// p = z + beta p, beta = r.z of iteration it + 1 over r.z of iteration it (first: p = z)
__global__ void __launch_bounds__(256) k_dyn_direction(int64_t n, const double *__restrict__ z, double *__restrict__ p, DynGate g, int first) {
    if (dyn_closed(g)) return;
    double beta = 0.0;
    if (!first) {
        const double *sc = g.scal + (int64_t)(g.it + (int)g.stop[3]) * 4;
        beta = sc[4] / sc[0];
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = first ? z[i] : fma(beta, p[i], z[i]);
}

// z = Dinv r, one lane per block row (test hook mfh_debug_pencil_precond: the blocks of k_pencil_dinv as a map; the loops apply them inside
// k_dyn_init / k_dyn_update and their complex counterparts)
template <int DIM>
__global__ void __launch_bounds__(256) k_pencil_apply(int64_t nRows, const double *__restrict__ dinv, const double *__restrict__ r, double *__restrict__ z) {
    constexpr int NS = DIM * (DIM + 1) / 2;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < nRows; n += (int64_t)gridDim.x * 256) {
        double rv[DIM], zv[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) rv[c] = r[n * DIM + c];
        apply_packed<DIM>(dinv + n * NS, rv, zv);
#pragma unroll
        for (int c = 0; c < DIM; ++c) z[n * DIM + c] = zv[c];
    }
}

void launch_newmark_predict(const PredictArgs &p, const double *u, const double *v, const double *a, const uint8_t *mask, double *ut, double *vt, double *xm,
                            double *xk, hipStream_t s) {
    hipLaunchKernelGGL(k_newmark_predict, dim3(dyn_grid(p.n)), dim3(256), 0, s, p, u, v, a, mask, ut, vt, xm, xk);
    CHECK_LAUNCH();
}

int launch_newmark_rhs(int64_t n, double g, const double *f, const double *y, const uint8_t *mask, double *b, double *partials, hipStream_t s) {
    const int grid = dyn_grid(n);
    hipLaunchKernelGGL(k_newmark_rhs, dim3(grid), dim3(256), 0, s, n, g, f, y, mask, b, partials);
    CHECK_LAUNCH();
    return grid;
}

void launch_newmark_correct(const CorrectArgs &p, const double *x, const double *ut, const double *vt, double *u, double *v, double *a, hipStream_t s) {
    hipLaunchKernelGGL(k_newmark_correct, dim3(dyn_grid(p.n)), dim3(256), 0, s, p, x, ut, vt, u, v, a);
    CHECK_LAUNCH();
}

}   // namespace
}}   // namespace mfh::k

using namespace mfh;
using namespace mfhi;
using k::DynGate;
using k::DYN_NV;

namespace {

struct NewmarkWork : PencilWork {
    double *u, *v, *a, *ut, *vt, *xm, *xk, *f, *b, *x, *r, *z, *p, *Ap;
    double rtol = 0, cK = 0, cM = 0;   // the tolerance set_threshold applies; the pencil of the solve under way

    // y = cK K x + cM M x on the free variables; dst (may be null) = x . y
    void pencil(const double *xin, double *y, double *dotDst, const DynGate &g) {
        lap(-1);
        if (cK != 0.0) apply_operator(c, masked, xin, y, nullptr);
        lap(0);
        const int np = k::launch_spmv_kron_acc(mass_spmv_args(c, masked), cK != 0.0, cK, cM, xin, y, dotDst ? partials.p : nullptr, g, s, c->dynGridCap);
        if (dotDst) sum_to(np, g, dotDst);
        lap(1);
    }
    template <bool BJ> void launch_init() {
        const int grid = vec_grid(nRows);
        k::with_dim(d, [&](auto D) {
            k::launch_k(k::k_dyn_init<D(), BJ>, dim3(grid), dim3(256), 0, s, nRows, (const double *)dinv.p, (const double *)b, (const double *)Ap, (const double *)bb, x, r, z, p, partials.p);
        });
        CHECK_LAUNCH();
        sum_to(grid, k::dyn_open(), BJ ? scal.p : nullptr, scal.p + 2);
    }
    template <bool BJ> void launch_update(int it) {
        const int grid = vec_grid(nRows);
        const DynGate g = gate(it);
        k::with_dim(d, [&](auto D) {
            k::launch_k(k::k_dyn_update<D(), BJ>, dim3(grid), dim3(256), 0, s, nRows, (const double *)dinv.p, (const double *)Ap, (const double *)p, x, r, z, g, partials.p);
        });
        CHECK_LAUNCH();
        sum_to(grid, g, BJ ? scal.p + (size_t)(it + 1) * 4 : nullptr, scal.p + (size_t)(it + 1) * 4 + 2);
    }
    // z = B r with the hierarchy of K (B ~ K^-1: its scaling by 1 / cK changes no PCG iterate and is left out), then r . z of iteration it + 1
    void coarse_precond(int it) {
        const DynGate g = it >= 0 ? gate(it) : k::dyn_open();
        if (useMG) mg_precond(c, r, z, it >= 0 ? scal.p : nullptr, it, it >= 0 ? stop : nullptr);
        else tl_precond(c, r, z, nullptr, -1);
        const int grid = vec_grid(n);
        hipLaunchKernelGGL(k::k_dyn_rz, dim3(grid), dim3(256), 0, s, n, (const double *)r, z, mask, g, partials.p);
        CHECK_LAUNCH();
        sum_to(grid, g, scal.p + (size_t)(it + 1) * 4);
    }
    void direction(int it, bool first) {
        hipLaunchKernelGGL(k::k_dyn_direction, dim3(vec_grid(n)), dim3(256), 0, s, n, (const double *)z, p, first ? k::dyn_open() : gate(it), first ? 1 : 0);
        CHECK_LAUNCH();
    }

    // the two halves of a PCG solve that pencil_loop calls: r = b - A x with the first z and p, and iteration `it`
    void start(bool jacobi) {
        if (jacobi) ensure_dinv(cK, cM);
        pencil(x, Ap, nullptr, k::dyn_open());
        if (jacobi) launch_init<true>();
        else { launch_init<false>(); coarse_precond(-1); direction(-1, true); }
    }
    void iterate(int it, bool jacobi) {
        pencil(p, Ap, scal.p + (size_t)it * 4 + 1, gate(it));
        if (jacobi) { launch_update<true>(it); lap(2); }
        else { launch_update<false>(it); lap(2); coarse_precond(it); lap(3); }
        direction(it, false);
        lap(4);
    }
    // PCG on A = cK K + cM M: b in this->b with b . b in bb[0] and the threshold in stop[0] (set_threshold), the start vector in x. Returns the
    // iterations taken, -1: maxit reached (x then holds the last iterate), -2: breakdown (a residual norm is not finite).
    int solve(double cK, double cM, bool jacobi) {
        this->cK = cK; this->cM = cM;
        return pencil_loop(*this, jacobi, batch, [&] { return batch = std::max(2, std::min(2 * batch, c->checkEvery)); }, true);
    }
    // b . b of the right-hand side just formed (the partials of k_newmark_rhs) -> bb[0] and the threshold rtol^2 b . b -> stop[0]
    void set_threshold(int nPart) {
        const int col[2] = {0, 0};
        const double sc[2] = {rtol * rtol, 1.0};
        double *const dst[2] = {stop, bb};
        reduce(nPart, 2, col, sc, dst, k::dyn_open());
    }
};

// What mfh_newmark and the test hooks of its loop (mfh_debug_pencil_precond, mfh_debug_newmark_pcg) share: setup_pencil_work and the work vectors
// of NewmarkWork::solve. Returns whether the time steps run block-Jacobi.
bool setup_newmark_work(mfh_ctx *c, NewmarkWork &w, const char *who, int maxit, double rtol) {
    const bool stepJacobi = setup_pencil_work(c, w, who, maxit);
    w.rtol = rtol;
    w.vec.alloc((size_t)w.ld * 14);
    w.vec.zero(w.s);
    double *q = w.vec.p;
    double **slots[14] = {&w.u, &w.v, &w.a, &w.ut, &w.vt, &w.xm, &w.xk, &w.f, &w.b, &w.x, &w.r, &w.z, &w.p, &w.Ap};
    for (auto sl : slots) { *sl = q; q += w.ld; }
    return stepJacobi;
}

void check_params(const mfh_newmark_params *p) {
    require(p != nullptr, MFH_ERR_INVALID, "mfh_newmark: params is null");
    require(p->dt > 0.0 && std::isfinite(p->dt), MFH_ERR_INVALID, "mfh_newmark: dt > 0");
    require(p->beta > 0.0 && std::isfinite(p->beta), MFH_ERR_INVALID, "mfh_newmark: beta > 0");
    require(p->gamma >= 0.5 && std::isfinite(p->gamma), MFH_ERR_INVALID, "mfh_newmark: gamma >= 1/2");
    require(p->density > 0.0 && std::isfinite(p->density), MFH_ERR_INVALID, "mfh_newmark: density > 0");
    require(p->rayleighMass >= 0.0 && p->rayleighStiff >= 0.0 && std::isfinite(p->rayleighMass) && std::isfinite(p->rayleighStiff), MFH_ERR_INVALID,
            "mfh_newmark: the Rayleigh coefficients are not negative");
    require(p->rtol > 0.0 && p->rtol < 1.0, MFH_ERR_INVALID, "mfh_newmark: 0 < rtol < 1");
    require(p->nSteps >= 0 && p->maxit > 0 && p->snapshotStride >= 0, MFH_ERR_INVALID, "mfh_newmark: nSteps >= 0, maxit > 0, snapshotStride >= 0");
    require((p->flags & ~(MFH_DYN_HAVE_ACCEL | MFH_DYN_ENERGIES)) == 0, MFH_ERR_INVALID, "mfh_newmark: unknown flag");
}

// y = (one double per block, kron I) x for host or device vectors of dim * nDoF entries (mfh_mass_apply, mfh_geometric_apply)
void kron_apply(mfh_ctx *c, const k::SpmvArgs &args, const double *x, double *y, int32_t flags) {
    hipStream_t s = c->stream;
    const bool onDevice = (flags & MFH_LOAD_ON_DEVICE) != 0;
    const int64_t n = (int64_t)c->mesh.dim * c->nDoF;
    DBuf<double> dx, dy;
    const double *xin = x;
    double *yout = y;
    if (!onDevice) {
        dx.alloc((size_t)n); dy.alloc((size_t)n);
        upload(dx.p, x, n, s);
        xin = dx.p; yout = dy.p;
    }
    k::launch_spmv_kron_acc(args, false, 0.0, 1.0, xin, yout, nullptr, k::dyn_open(), s, c->dynGridCap);
    if (!onDevice) MFH_HIP(hipMemcpyAsync(y, dy.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
}

}   // namespace

extern "C" {

mfh_status mfh_newmark(mfh_ctx *c, const mfh_newmark_params *prm, double *u, double *v, double *a, const double *f, const double *amplitude,
                       const int64_t *probeVars, int32_t nProbe, double *probeOut, double *snapshots, double *energies, mfh_newmark_info *info) {
    if (info) { *info = mfh_newmark_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_newmark: null context");
    check_params(prm);
    const mfh_newmark_params P = *prm;
    require(u && v && a, MFH_ERR_INVALID, "mfh_newmark: u, v and a are not null");
    require(nProbe >= 0 && (nProbe == 0 || (probeVars && probeOut)), MFH_ERR_INVALID, "mfh_newmark: probes need their variables and their output");
    const bool wantE = (P.flags & MFH_DYN_ENERGIES) != 0;
    require(!energies || wantE, MFH_ERR_INVALID, "mfh_newmark: energies given without MFH_DYN_ENERGIES");
    require(!wantE || energies, MFH_ERR_INVALID, "mfh_newmark: MFH_DYN_ENERGIES needs the energies array");
    require(!snapshots || P.snapshotStride > 0, MFH_ERR_INVALID, "mfh_newmark: snapshots need snapshotStride > 0");
    {
        const int64_t nv = (int64_t)c->bs() * c->nDoF;
        for (int32_t j = 0; j < nProbe; ++j) require(probeVars[j] >= 0 && probeVars[j] < nv, MFH_ERR_INVALID, "mfh_newmark: probe variable out of range");
    }
    prepare_pencil(c, "mfh_newmark");
    hipStream_t s = c->stream;
    c->dynNote.clear();
    auto note = [&](const std::string &t) { if (!c->dynNote.empty()) c->dynNote += "; "; c->dynNote += t; };
    WideGuard guard(c);
    if (guard.widened) note("the pattern held the upper triangle only: symbolic phase re-run with both triangles (what option matrix_storage 0 does) for this call");
    if (2.0 * P.beta < P.gamma) note("2 beta < gamma: the scheme is only conditionally stable");
    EventTimer tsetup(s);
    const bool masked = !c->fixedVars.empty();
    const double bdt = P.beta * P.dt;
    const double cK = 1.0 + P.gamma * P.rayleighStiff / bdt;
    const double cM = P.density * (1.0 / (bdt * P.dt) + P.gamma * P.rayleighMass / bdt);
    NewmarkWork w;
    const bool stepJacobi = setup_newmark_work(c, w, "mfh_newmark", P.maxit, P.rtol);
    if (w.wantCoarse && !masked) note("no fixed variables (K singular, A not): block-Jacobi of A in place of the two-level / multigrid preconditioner");
    else if (w.wantCoarse && stepJacobi) note(c->precondNote.empty() ? std::string("two-level / multigrid preconditioner unavailable: block-Jacobi of A") : c->precondNote + " (block-Jacobi of A)");
    else if (!w.wantCoarse) note("block-Jacobi of A = cK K + cM M");
    else if (w.useTL && c->precond == MFH_PRECOND_MULTIGRID) note(c->precondNote.empty() ? std::string("multigrid hierarchy unavailable: two-level preconditioner of K") : c->precondNote);

    const int nSteps = P.nSteps;
    const int stride = snapshots ? P.snapshotStride : 0;
    const int64_t nSnapRows = stride ? nSteps / stride + 1 : 0;
    // snapshot rows wait on the device and leave in groups (256 MB at most, one row at least)
    const int64_t snapCap = stride ? std::max<int64_t>(1, std::min<int64_t>(nSnapRows, ((int64_t)1 << 25) / std::max<int64_t>(w.n, 1))) : 0;
    DBuf<double> dSnap, dProbe, dEnergy;
    DBuf<int64_t> dProbeVars;
    if (stride) dSnap.alloc((size_t)snapCap * (size_t)w.n);
    if (nProbe) {
        dProbe.alloc((size_t)(nSteps + 1) * (size_t)nProbe);
        dProbeVars.alloc((size_t)nProbe);
        MFH_HIP(hipMemcpyAsync(dProbeVars.p, probeVars, (size_t)nProbe * sizeof(int64_t), hipMemcpyHostToDevice, s));
    }
    if (wantE) { dEnergy.alloc((size_t)(nSteps + 1) * 3); dEnergy.zero(s); }
    upload(w.u, u, w.n, s);
    upload(w.v, v, w.n, s);
    if (P.flags & MFH_DYN_HAVE_ACCEL) upload(w.a, a, w.n, s);
    if (f) upload(w.f, f, w.n, s);
    if (masked) { k::launch_mask(w.n, w.mask, w.u, s); k::launch_mask(w.n, w.mask, w.v, s); k::launch_mask(w.n, w.mask, w.a, s); }
    MFH_HIP(hipStreamSynchronize(s));
    const double setupMs = tsetup.stop();

    EventTimer tsolve(s);
    int stepsDone = 0, itTotal = 0, itMax = 0, itInit = 0;
    int64_t snapHeld = 0, snapWritten = 0;
    auto flush_snapshots = [&]() {
        if (snapHeld) MFH_HIP(hipMemcpyAsync(snapshots + (size_t)snapWritten * (size_t)w.n, dSnap.p, (size_t)snapHeld * (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
        MFH_HIP(hipStreamSynchronize(s));
        snapWritten += snapHeld;
        snapHeld = 0;
    };
    // probe values, snapshot row and energies of the state (u, v) at step `step`; x: the solution the correction reads (null: record only)
    auto finish_step = [&](int step, const double *x) {
        k::CorrectArgs ca{};
        ca.n = w.n; ca.ca = 1.0 / (bdt * P.dt); ca.cv = P.gamma * P.dt; ca.recordOnly = x ? 0 : 1;
        ca.nProbe = nProbe; ca.probeVars = dProbeVars.p; ca.probeRow = nProbe ? dProbe.p + (size_t)step * (size_t)nProbe : nullptr;
        if (stride && step % stride == 0) {
            if (snapHeld == snapCap) flush_snapshots();
            ca.snapRow = dSnap.p + (size_t)snapHeld * (size_t)w.n;
            ++snapHeld;
        }
        k::launch_newmark_correct(ca, x ? x : w.u, w.ut, w.vt, w.u, w.v, w.a, s);
        if (wantE) {
            const double g = amplitude ? amplitude[step] : 1.0;
            double *row = dEnergy.p + (size_t)step * 3;
            // kinetic: 1/2 v . (density M) v through the accumulate kernel's dot; strain and work: K u, then {u . K u, f . u}
            const int np = k::launch_spmv_kron_acc(mass_spmv_args(c, masked), false, 0.0, P.density, w.v, w.r, w.partials.p, k::dyn_open(), s, c->dynGridCap);
            { const int col[1] = {0}; const double sc[1] = {0.5}; double *const dst[1] = {row}; w.reduce(np, 1, col, sc, dst, k::dyn_open()); }
            apply_operator(c, masked, w.u, w.r, nullptr);
            const int grid = w.vec_grid(w.n);
            hipLaunchKernelGGL(k::k_dyn_dot2, dim3(grid), dim3(256), 0, s, w.n, (const double *)w.u, (const double *)w.r, f ? (const double *)w.f : (const double *)nullptr, w.partials.p);
            CHECK_LAUNCH();
            { const int col[2] = {0, 1}; const double sc[2] = {0.5, g}; double *const dst[2] = {row + 1, row + 2}; w.reduce(grid, 2, col, sc, dst, k::dyn_open()); }
        }
    };
    mfh_status failure = MFH_OK;
    std::string failText;
    bool step0Done = (P.flags & MFH_DYN_HAVE_ACCEL) != 0;
    // ---- a0 from M a0 = g0 f - C v0 - K u0: the pencil solve with cK = 0, block-Jacobi of density M
    if (!(P.flags & MFH_DYN_HAVE_ACCEL)) {
        const double g0 = amplitude ? amplitude[0] : 1.0;
        // xm = -density aR v0 (M multiplies it), xk = -(u0 + bR v0) (K multiplies it)
        MFH_HIP(hipMemcpyAsync(w.xm, w.v, (size_t)w.n * sizeof(double), hipMemcpyDeviceToDevice, s));
        k::launch_axpby(w.n, 0.0, w.xm, -P.density * P.rayleighMass, w.xm, s);
        MFH_HIP(hipMemcpyAsync(w.xk, w.u, (size_t)w.n * sizeof(double), hipMemcpyDeviceToDevice, s));
        k::launch_axpby(w.n, -P.rayleighStiff, w.v, -1.0, w.xk, s);
        apply_operator(c, masked, w.xk, w.Ap, nullptr);
        k::launch_spmv_kron_acc(mass_spmv_args(c, masked), true, 1.0, 1.0, w.xm, w.Ap, nullptr, k::dyn_open(), s, c->dynGridCap);
        const int np = k::launch_newmark_rhs(w.n, g0, f ? w.f : nullptr, w.Ap, w.mask, w.b, w.partials.p, s);
        w.set_threshold(np);
        MFH_HIP(hipMemsetAsync(w.x, 0, (size_t)w.n * sizeof(double), s));
        const int its = w.solve(0.0, P.density, true);
        if (its < 0) {
            failure = MFH_ERR_NOT_CONVERGED;
            failText = its == -1 ? "mfh_newmark: the PCG for the initial acceleration reached maxit" : "mfh_newmark: PCG breakdown in the solve for the initial acceleration";
        } else {
            itInit = its;
            step0Done = true;
            MFH_HIP(hipMemcpyAsync(w.a, w.x, (size_t)w.n * sizeof(double), hipMemcpyDeviceToDevice, s));
        }
    }
    if (failure == MFH_OK) {
        finish_step(0, nullptr);
        k::PredictArgs pa{};
        pa.n = w.n; pa.dt = P.dt; pa.cua = P.dt * P.dt * (0.5 - P.beta); pa.cva = P.dt * (1.0 - P.gamma);
        pa.cw = P.gamma / bdt; pa.cmu = P.density / (bdt * P.dt); pa.cmw = P.density * P.rayleighMass; pa.ckw = P.rayleighStiff;
        const bool haveCK = P.rayleighStiff != 0.0;
        for (int step = 1; step <= nSteps; ++step) {
            const double g = amplitude ? amplitude[step] : 1.0;
            w.lap(-1);
            k::launch_newmark_predict(pa, w.u, w.v, w.a, w.mask, w.ut, w.vt, w.xm, haveCK ? w.xk : nullptr, s);
            if (haveCK) apply_operator(c, masked, w.xk, w.Ap, nullptr);
            k::launch_spmv_kron_acc(mass_spmv_args(c, masked), haveCK, 1.0, 1.0, w.xm, w.Ap, nullptr, k::dyn_open(), s, c->dynGridCap);
            const int np = k::launch_newmark_rhs(w.n, g, f ? w.f : nullptr, w.Ap, w.mask, w.b, w.partials.p, s);
            w.set_threshold(np);
            MFH_HIP(hipMemcpyAsync(w.x, w.ut, (size_t)w.n * sizeof(double), hipMemcpyDeviceToDevice, s));      // warm start
            w.lap(6);
            const int its = w.solve(cK, cM, stepJacobi);
            if (its < 0) {
                failure = MFH_ERR_NOT_CONVERGED;
                failText = its == -1 ? "mfh_newmark: the PCG of step " + std::to_string(step) + " reached maxit" : "mfh_newmark: PCG breakdown in step " + std::to_string(step);
                break;
            }
            itTotal += its;
            itMax = std::max(itMax, its);
            w.lap(-1);
            finish_step(step, w.x);
            w.lap(6);
            stepsDone = step;
        }
    }
    if (stride) flush_snapshots();
    if (step0Done) {        // (a failed solve for a0 leaves the caller's arrays as they were)
        MFH_HIP(hipMemcpyAsync(u, w.u, (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
        MFH_HIP(hipMemcpyAsync(v, w.v, (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
        MFH_HIP(hipMemcpyAsync(a, w.a, (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
        const size_t rows = (size_t)stepsDone + 1;
        if (nProbe) MFH_HIP(hipMemcpyAsync(probeOut, dProbe.p, rows * (size_t)nProbe * sizeof(double), hipMemcpyDeviceToHost, s));
        if (wantE) MFH_HIP(hipMemcpyAsync(energies, dEnergy.p, rows * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    MFH_HIP(hipStreamSynchronize(s));
    const double solveMs = tsolve.stop();
    if (w.timing)
        fprintf(stderr, "[mfh_newmark] n %lld steps %d iterations %d | ms: K %.3f M %.3f update %.3f precond %.3f direction %.3f readback %.3f step-kernels %.3f\n",
                (long long)w.n, stepsDone, itTotal, w.tPhase[0], w.tPhase[1], w.tPhase[2], w.tPhase[3], w.tPhase[4], w.tPhase[5], w.tPhase[6]);
    if (info) {
        info->stepsDone = stepsDone;
        info->iterationsTotal = itTotal;
        info->iterationsMax = itMax;
        info->iterationsInit = itInit;
        info->precondUsed = w.useMG ? MFH_PRECOND_MULTIGRID : (w.useTL ? MFH_PRECOND_TWO_LEVEL : MFH_PRECOND_BLOCK_JACOBI);
        info->cK = cK; info->cM = cM;
        info->solve_ms = solveMs; info->setup_ms = setupMs;
        info->note = c->dynNote.c_str();
    }
    if (failure != MFH_OK) throw Error(failure, failText);
    MFH_CATCH(c)
}

// ---- test hooks (include/meshfem_hip_extras.h): the step kernels on host arrays, the pencil product on the context's operators
mfh_status mfh_debug_newmark_predict(mfh_ctx *c, int64_t n, double dt, double beta, double gamma, double density, double rayleighMass, double rayleighStiff,
                                     const uint8_t *mask, const double *u, const double *v, const double *a, double *ut, double *vt, double *xm, double *xk) {
    MFH_TRY(c)
    require(c && n >= 1 && u && v && a && ut && vt && xm && dt > 0 && beta > 0, MFH_ERR_INVALID, "mfh_debug_newmark_predict: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DBuf<double> in, out;
    DBuf<uint8_t> dm;
    in.alloc((size_t)n * 3); out.alloc((size_t)n * 4);
    upload(in.p, u, n, s); upload(in.p + n, v, n, s); upload(in.p + 2 * n, a, n, s);
    if (mask) dm.upload(mask, (size_t)n, s);
    k::PredictArgs pa{};
    const double bdt = beta * dt;
    pa.n = n; pa.dt = dt; pa.cua = dt * dt * (0.5 - beta); pa.cva = dt * (1.0 - gamma);
    pa.cw = gamma / bdt; pa.cmu = density / (bdt * dt); pa.cmw = density * rayleighMass; pa.ckw = rayleighStiff;
    k::launch_newmark_predict(pa, in.p, in.p + n, in.p + 2 * n, mask ? dm.p : nullptr, out.p, out.p + n, out.p + 2 * n, xk ? out.p + 3 * n : nullptr, s);
    MFH_HIP(hipMemcpyAsync(ut, out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(vt, out.p + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(xm, out.p + 2 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (xk) MFH_HIP(hipMemcpyAsync(xk, out.p + 3 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

mfh_status mfh_debug_newmark_rhs(mfh_ctx *c, int64_t n, double g, const double *f, const double *y, const uint8_t *mask, double *b, double *bb) {
    MFH_TRY(c)
    require(c && n >= 1 && y && b && bb, MFH_ERR_INVALID, "mfh_debug_newmark_rhs: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DBuf<double> in, out, part;
    DBuf<uint8_t> dm;
    in.alloc((size_t)n * 2); out.alloc((size_t)n + 1); part.alloc((size_t)k::DYN_GRID_CAP * DYN_NV);
    upload(in.p, y, n, s);
    if (f) upload(in.p + n, f, n, s);
    if (mask) dm.upload(mask, (size_t)n, s);
    const int np = k::launch_newmark_rhs(n, g, f ? in.p + n : nullptr, in.p, mask ? dm.p : nullptr, out.p, part.p, s);
    k::launch_sum(np, part.p, k::dyn_open(), s, out.p + n);
    MFH_HIP(hipMemcpyAsync(b, out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(bb, out.p + n, sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

mfh_status mfh_debug_newmark_correct(mfh_ctx *c, int64_t n, double dt, double beta, double gamma, const double *x, const double *ut, const double *vt,
                                     double *u, double *v, double *a, const int64_t *probeVars, int32_t nProbe, double *probeOut, double *snapshot) {
    MFH_TRY(c)
    require(c && n >= 1 && x && ut && vt && u && v && a && dt > 0 && beta > 0 && nProbe >= 0 && (nProbe == 0 || (probeVars && probeOut)), MFH_ERR_INVALID,
            "mfh_debug_newmark_correct: arguments");
    for (int32_t j = 0; j < nProbe; ++j) require(probeVars[j] >= 0 && probeVars[j] < n, MFH_ERR_INVALID, "mfh_debug_newmark_correct: probe variable out of range");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DBuf<double> in, out;
    DBuf<int64_t> dv;
    in.alloc((size_t)n * 3); out.alloc((size_t)n * 4 + (size_t)std::max(nProbe, 1));
    upload(in.p, x, n, s); upload(in.p + n, ut, n, s); upload(in.p + 2 * n, vt, n, s);
    if (nProbe) { dv.alloc((size_t)nProbe); MFH_HIP(hipMemcpyAsync(dv.p, probeVars, (size_t)nProbe * sizeof(int64_t), hipMemcpyHostToDevice, s)); }
    k::CorrectArgs ca{};
    ca.n = n; ca.ca = 1.0 / (beta * dt * dt); ca.cv = gamma * dt; ca.recordOnly = 0;
    ca.nProbe = nProbe; ca.probeVars = dv.p; ca.probeRow = nProbe ? out.p + 4 * n : nullptr;
    ca.snapRow = snapshot ? out.p + 3 * n : nullptr;
    k::launch_newmark_correct(ca, in.p, in.p + n, in.p + 2 * n, out.p, out.p + n, out.p + 2 * n, s);
    MFH_HIP(hipMemcpyAsync(u, out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(v, out.p + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(a, out.p + 2 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (snapshot) MFH_HIP(hipMemcpyAsync(snapshot, out.p + 3 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (nProbe) MFH_HIP(hipMemcpyAsync(probeOut, out.p + 4 * n, (size_t)nProbe * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

// y = M x on displacement vectors, unmasked: the resident mass buffer (the context's density field in it) through k_spmv_kron_acc
mfh_status mfh_mass_apply(mfh_ctx *c, const double *x, double *y, int32_t flags) {
    MFH_TRY(c)
    require(c && x && y, MFH_ERR_INVALID, "mfh_mass_apply: null argument");
    require((flags & ~MFH_LOAD_ON_DEVICE) == 0, MFH_ERR_INVALID, "flags: 0 | MFH_LOAD_ON_DEVICE");
    require(c->haveMesh && !c->hostOnly && !c->external, MFH_ERR_STATE, "the resident mass matrix needs a mesh on a device");
    prepare_pencil(c, "mfh_mass_apply");
    WideGuard guard(c);
    ensure_mass(c);
    kron_apply(c, mass_spmv_args(c, false), x, y, flags);
    MFH_CATCH(c)
}

// y = Kg x on displacement vectors, unmasked: the resident geometric stiffness of the context's prestress, the same way
mfh_status mfh_geometric_apply(mfh_ctx *c, const double *x, double *y, int32_t flags) {
    MFH_TRY(c)
    require(c && x && y, MFH_ERR_INVALID, "mfh_geometric_apply: null argument");
    require((flags & ~MFH_LOAD_ON_DEVICE) == 0, MFH_ERR_INVALID, "flags: 0 | MFH_LOAD_ON_DEVICE");
    require(c->haveMesh && !c->hostOnly && !c->external, MFH_ERR_STATE, "the resident geometric stiffness needs a mesh on a device");
    prepare_pencil(c, "mfh_geometric_apply");
    require(c->havePrestress, MFH_ERR_STATE, "mfh_geometric_apply: no prestress field set (mfh_set_prestress / mfh_prestress_from_displacement)");
    WideGuard guard(c);
    ensure_geometric(c);
    kron_apply(c, geom_spmv_args(c, false), x, y, flags);
    MFH_CATCH(c)
}

mfh_status mfh_debug_pencil_apply(mfh_ctx *c, double cK, double cM, int32_t masked, const double *x, double *y, double *dot) {
    MFH_TRY(c)
    require(c && x && y && std::isfinite(cK) && std::isfinite(cM), MFH_ERR_INVALID, "mfh_debug_pencil_apply: arguments");
    prepare_pencil(c, "mfh_debug_pencil_apply");
    hipStream_t s = c->stream;
    WideGuard guard(c);
    prepare_pencil_state(c, "mfh_debug_pencil_apply", false);
    const int64_t n = (int64_t)c->bs() * c->nDoF;
    const bool m = masked != 0 && !c->fixedVars.empty();
    DBuf<double> dx, dy, part;
    dx.alloc((size_t)n); dy.alloc((size_t)n + 1); part.alloc((size_t)k::DYN_GRID_CAP * DYN_NV);
    upload(dx.p, x, n, s);
    if (cK != 0.0) apply_operator(c, m, dx.p, dy.p, nullptr);
    const int np = k::launch_spmv_kron_acc(mass_spmv_args(c, m), cK != 0.0, cK, cM, dx.p, dy.p, part.p, k::dyn_open(), s, c->dynGridCap);
    k::launch_sum(np, part.p, k::dyn_open(), s, dy.p + n);
    MFH_HIP(hipMemcpyAsync(y, dy.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (dot) MFH_HIP(hipMemcpyAsync(dot, dy.p + n, sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

// z = Dinv r with the blocks PencilWork::ensure_dinv builds for (cK, cM) (the Newmark loop's call; the harmonic loop asks for cK = 1)
mfh_status mfh_debug_pencil_precond(mfh_ctx *c, double cK, double cM, const double *r, double *z) {
    MFH_TRY(c)
    require(c && r && z && std::isfinite(cK) && std::isfinite(cM), MFH_ERR_INVALID, "mfh_debug_pencil_precond: arguments");
    prepare_pencil(c, "mfh_debug_pencil_precond");
    hipStream_t s = c->stream;
    WideGuard guard(c);
    // the whole setup of the loop for one block apply, deliberately: ensure_dinv then sees the context in the state the loop's own call sees it in
    // (storage, assembled K, mass buffer, mask)
    NewmarkWork w;
    setup_newmark_work(c, w, "mfh_debug_pencil_precond", 1, 0.5);
    w.ensure_dinv(cK, cM);
    upload(w.r, r, w.n, s);
    k::with_dim(w.d, [&](auto D) {
        k::launch_k(k::k_pencil_apply<D()>, dim3(k::dyn_grid(w.nRows)), dim3(256), 0, s, w.nRows, (const double *)w.dinv.p, (const double *)w.r, w.z);
    });
    CHECK_LAUNCH();
    MFH_HIP(hipMemcpyAsync(z, w.z, (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

// NewmarkWork::solve on (b, x0) as a time step of mfh_newmark calls it: b masked and its threshold set by k_newmark_rhs / set_threshold, the
// preconditioner the steps would take (cK == 0: block-Jacobi of cM M, the solve for the initial acceleration)
mfh_status mfh_debug_newmark_pcg(mfh_ctx *c, double cK, double cM, double rtol, int32_t maxit, const double *b, const double *x0, double *x, double *history,
                                 int32_t *its) {
    MFH_TRY(c)
    require(c && b && x && history && its && std::isfinite(cK) && std::isfinite(cM) && rtol > 0.0 && rtol < 1.0 && maxit > 0, MFH_ERR_INVALID,
            "mfh_debug_newmark_pcg: arguments");
    prepare_pencil(c, "mfh_debug_newmark_pcg");
    hipStream_t s = c->stream;
    WideGuard guard(c);
    NewmarkWork w;
    const bool stepJacobi = setup_newmark_work(c, w, "mfh_debug_newmark_pcg", maxit, rtol);
    upload(w.f, b, w.n, s);
    const int np = k::launch_newmark_rhs(w.n, 0.0, nullptr, w.f, w.mask, w.b, w.partials.p, s);
    w.set_threshold(np);
    if (x0) upload(w.x, x0, w.n, s);           // (zero on the fixed variables, as k_newmark_predict leaves the loop's start vector)
    const int ret = w.solve(cK, cM, cK == 0.0 || stepJacobi);
    MFH_HIP(hipMemcpyAsync(x, w.x, (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(history, w.scal.p, ((size_t)maxit + 1) * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    *its = ret;
    if (ret < 0) throw Error(MFH_ERR_NOT_CONVERGED, ret == -1 ? "mfh_debug_newmark_pcg: the PCG reached maxit" : "mfh_debug_newmark_pcg: PCG breakdown");
    MFH_CATCH(c)
}

}   // extern "C"
