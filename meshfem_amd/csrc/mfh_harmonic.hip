// Frequency response (mfh_harmonic, include/meshfem_hip.h; docs/design/04_17_harmonic.md): the steady state u^(w) of M u'' + C u' + K u = Re(f^ e^{iwt}),
//   Z(w) u^ = f^,   Z = zK K + zM M,   zK = 1 + i (eta + w bR),   zM = density (-w^2 + i w aR),   fixed variables held at zero,
// for a list of frequencies. Z is complex SYMMETRIC (not Hermitian): the solver is COCG, the PCG recurrence of mfh_dynamics.hip with the unconjugated
// bilinear form x^T y in place of the inner product, preconditioned by a REAL symmetric positive-definite B applied to the two planes: K's two-level /
// multigrid hierarchy, or the block-Jacobi of K + w^2 density M (k_pencil_dinv, rebuilt when w changes). A complex vector is two real planes
// (re at v, im at v + ld) because apply_operator, tl_precond and mg_precond take real vectors.
//   k_spmv_kron_cacc   y = zK y + zM (M (x) I) x on both planes: k_spmv_kron_acc's chunk walk, every stored mass value and column index loaded ONCE, LDS
//                      partials [2 dim][chunkSlots]; the two neighbouring lanes that finish the planes of a scalar row exchange their sums, combine
//                      them with the two K products apply_operator left in y, zero the fixed rows and add the two parts of x^T y to the workgroup's
//                      partial (zK == 0: y is not read)
//   k_harm_combine     the same combination from two real products (two launches of k_spmv_kron_acc): the form the launcher takes where the 2 dim
//                      planes of partials exceed the LDS, or under option harmonic_two_pass
//   k_harm_*           the COCG's vector kernels; alpha = (r^T z) / (p^T Z p) and beta are formed on the device from the history
// Histories: scal[4 it + 2] = the Hermitian r . r with the control block of mfh_dynamics.hip (what the gate and mg_precond read); the complex scalars
// in a second array, cs[4 it + {0, 1}] = r^T z, cs[4 it + {2, 3}] = p^T Z p. Sums as in mfh_pencil.hh: one plain-store partial per workgroup,
// k_dyn_reduce in a fixed order, no floating-point atomics, grids that depend on n and option dyn_grid_cap only.
#include "mfh_pencil.hh"

namespace mfh { namespace k {

namespace {

struct Cx { double re, im; };
DEV Cx cmul(const Cx &a, const Cx &b) { return Cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
DEV Cx cdiv(const Cx &a, const Cx &b) {
    const double d = b.re * b.re + b.im * b.im;
    return Cx{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
// the complex scalars of iteration it (+ the iteration base of the control block)
DEV const double *harm_cs(const DynGate &g, const double *cs) { return cs + (int64_t)(g.it + (int)g.stop[3]) * 4; }

// the row's value of Z x from its two products, and its part of x^T y (unconjugated)
template <bool ACC>
DEV void harm_row(const Cx &zK, const Cx &zM, const Cx &mx, const Cx &kx, const Cx &xv, bool fixed, Cx &yv, double *dot) {
    yv = cmul(zM, mx);
    if (ACC) { const Cx ky = cmul(zK, kx); yv.re += ky.re; yv.im += ky.im; }
    if (fixed) { yv.re = 0.0; yv.im = 0.0; }
    dot[0] += xv.re * yv.re - xv.im * yv.im;
    dot[1] += xv.re * yv.im + xv.im * yv.re;
}

template <int N, bool ACC>
__global__ void __launch_bounds__(256) k_spmv_kron_cacc(SpmvArgs a, Cx zK, Cx zM, const double *__restrict__ x, double *y, int64_t ld,
                                                       double *__restrict__ partials, DynGate g) {
    extern __shared__ __attribute__((aligned(16))) double part[];  // [2 N][chunkSlots] + 16
    const int CS = a.chunkSlots;
    double *red = part + 2 * N * CS;
    if (dyn_closed(g)) return;
    double dot[2] = {0.0, 0.0};
    for (int64_t chunk = blockIdx.x; chunk < a.nChunk; chunk += gridDim.x) {
        const int r0 = a.chunkRow[chunk], r1 = a.chunkRow[chunk + 1];
        const int s0 = a.rowPtr[r0];
        const int ns = a.rowPtr[r1] - s0;
        for (int t = threadIdx.x; t < ns; t += 256) {
            const int64_t s = (int64_t)s0 + t;
            const int64_t col = a.colIdx[s];
            const double m = a.vals[tiled_index(s, 0, 1)];
#pragma unroll
            for (int c = 0; c < N; ++c) {
                part[c * CS + t] = m * x[col * N + c];
                part[(N + c) * CS + t] = m * x[ld + col * N + c];
            }
        }
        __syncthreads();
        // a chunk of 512 slots holds some 50 scalar rows: one lane per (scalar row, plane), the two planes of a row in neighbouring lanes, so that
        // the serial walk over a row's partials is as long as k_spmv_kron_acc's and twice as many lanes walk. The neighbours then exchange their
        // sums, K products and x entries, and each writes its own plane of y and adds its own part of x^T y.
        const int nscalar = (r1 - r0) * N;
        for (int idx = threadIdx.x; idx < 2 * nscalar; idx += 256) {         // (256 is even: lanes 2 j and 2 j + 1 are in the loop together)
            const int plane = idx & 1, sidx = idx >> 1;
            const int rl = sidx / N, c = sidx - rl * N;
            const int64_t r = r0 + rl;
            const int b = a.rowPtr[r] - s0, e = a.rowPtr[r + 1] - s0;
            const double *pp = part + (plane * N + c) * CS;
            double m = 0.0;
            for (int t = b; t < e; ++t) m += pp[t];
            const int64_t gi = r * N + c, pi = plane * ld + gi;
            const double kv = ACC ? y[pi] : 0.0, xv = x[pi];
            const double mo = __shfl_xor(m, 1), ko = __shfl_xor(kv, 1), xo = __shfl_xor(xv, 1);
            Cx yv;
            double d2[2] = {0.0, 0.0};
            harm_row<ACC>(zK, zM, plane ? Cx{mo, m} : Cx{m, mo}, plane ? Cx{ko, kv} : Cx{kv, ko}, plane ? Cx{xo, xv} : Cx{xv, xo},
                          a.fixedMask && a.fixedMask[gi], yv, d2);
            y[pi] = plane ? yv.im : yv.re;
            dot[plane] += d2[plane];
        }
        __syncthreads();
    }
    store_partials<2>(dot, red, partials);
}

// y = zK y + zM t with t = (M xr, M xi) from two launches of k_spmv_kron_acc; the fixed rows zeroed; partials {Re, Im} of x^T y
template <bool ACC>
__global__ void __launch_bounds__(256) k_harm_combine(int64_t n, Cx zK, Cx zM, const double *__restrict__ x, double *__restrict__ y,
                                                     const double *__restrict__ t, int64_t ld, const uint8_t *__restrict__ mask,
                                                     double *__restrict__ partials, DynGate g) {
    __shared__ double red[8];
    if (dyn_closed(g)) return;
    double dot[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        Cx kx{0.0, 0.0}, yv;
        if (ACC) { kx.re = y[i]; kx.im = y[ld + i]; }
        harm_row<ACC>(zK, zM, Cx{t[i], t[ld + i]}, kx, Cx{x[i], x[ld + i]}, mask && mask[i], yv, dot);
        y[i] = yv.re;
        y[ld + i] = yv.im;
    }
    store_partials<2>(dot, red, partials);
}

// partials {|v|^2} over both planes
__global__ void __launch_bounds__(256) k_harm_norm2(int64_t n, const double *__restrict__ v, int64_t ld, double *__restrict__ partials) {
    __shared__ double red[8];
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double a = v[i], b = v[ld + i];
        acc[0] = fma(a, a, fma(b, b, acc[0]));
    }
    store_partials<1>(acc, red, partials);
}

// ---- the COCG's vector kernels (one lane per block row: DIM consecutive variables of both planes)
// r = b - Ax; BJ: z = Dinv r on both planes, p = z, partials {Re r^T z, Im r^T z, r . r}; else {-, -, r . r}
template <int DIM, bool BJ>
__global__ void __launch_bounds__(256) k_harm_init(int64_t nRows, const double *__restrict__ dinv, const double *__restrict__ b, const double *__restrict__ Ax,
                                                  double *__restrict__ r, double *__restrict__ z, double *__restrict__ p, int64_t ld,
                                                  double *__restrict__ partials) {
    __shared__ double red[16];
    constexpr int NS = DIM * (DIM + 1) / 2;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < nRows; n += (int64_t)gridDim.x * 256) {
        double rr[DIM], ri[DIM], zr[DIM], zi[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            const int64_t i = n * DIM + c;
            rr[c] = b[i] - Ax[i];
            ri[c] = b[ld + i] - Ax[ld + i];
            r[i] = rr[c];
            r[ld + i] = ri[c];
            acc[2] = fma(rr[c], rr[c], fma(ri[c], ri[c], acc[2]));
        }
        if (BJ) {
            apply_packed<DIM>(dinv + n * NS, rr, zr);
            apply_packed<DIM>(dinv + n * NS, ri, zi);
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                const int64_t i = n * DIM + c;
                z[i] = zr[c]; z[ld + i] = zi[c];
                p[i] = zr[c]; p[ld + i] = zi[c];
                acc[0] += rr[c] * zr[c] - ri[c] * zi[c];
                acc[1] += rr[c] * zi[c] + ri[c] * zr[c];
            }
        }
    }
    store_partials<3>(acc, red, partials);
}

// alpha = r^T z / p^T Z p of iteration it;  x += alpha p;  r -= alpha Ap;  BJ: z = Dinv r, partials {Re r^T z, Im r^T z, r . r}; else {-, -, r . r}
template <int DIM, bool BJ>
__global__ void __launch_bounds__(256) k_harm_update(int64_t nRows, const double *__restrict__ dinv, const double *__restrict__ Ap, const double *__restrict__ p,
                                                    double *__restrict__ x, double *__restrict__ r, double *__restrict__ z, int64_t ld, DynGate g,
                                                    const double *__restrict__ cs, double *__restrict__ partials) {
    __shared__ double red[16];
    constexpr int NS = DIM * (DIM + 1) / 2;
    if (dyn_closed(g)) return;
    const double *sc = harm_cs(g, cs);
    const Cx alpha = cdiv(Cx{sc[0], sc[1]}, Cx{sc[2], sc[3]});
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < nRows; n += (int64_t)gridDim.x * 256) {
        double rr[DIM], ri[DIM], zr[DIM], zi[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            const int64_t i = n * DIM + c;
            const Cx ap = cmul(alpha, Cx{p[i], p[ld + i]}), aq = cmul(alpha, Cx{Ap[i], Ap[ld + i]});
            x[i] += ap.re;
            x[ld + i] += ap.im;
            rr[c] = r[i] - aq.re;
            ri[c] = r[ld + i] - aq.im;
            r[i] = rr[c];
            r[ld + i] = ri[c];
            acc[2] = fma(rr[c], rr[c], fma(ri[c], ri[c], acc[2]));
        }
        if (BJ) {
            apply_packed<DIM>(dinv + n * NS, rr, zr);
            apply_packed<DIM>(dinv + n * NS, ri, zi);
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                const int64_t i = n * DIM + c;
                z[i] = zr[c]; z[ld + i] = zi[c];
                acc[0] += rr[c] * zr[c] - ri[c] * zi[c];
                acc[1] += rr[c] * zi[c] + ri[c] * zr[c];
            }
        }
    }
    store_partials<3>(acc, red, partials);
}

// after the two-level / multigrid preconditioner on both planes: z = r on the fixed variables (r is 0 there), partials {Re r^T z, Im r^T z}
__global__ void __launch_bounds__(256) k_harm_rz(int64_t n, const double *__restrict__ r, double *__restrict__ z, int64_t ld, const uint8_t *__restrict__ mask,
                                                DynGate g, double *__restrict__ partials) {
    __shared__ double red[8];
    if (dyn_closed(g)) return;
    double acc[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double rr = r[i], ri = r[ld + i];
        double zr = z[i], zi = z[ld + i];
        if (mask && mask[i]) { zr = rr; zi = ri; z[i] = zr; z[ld + i] = zi; }
        acc[0] += rr * zr - ri * zi;
        acc[1] += rr * zi + ri * zr;
    }
    store_partials<2>(acc, red, partials);
}

// p = z + beta p, beta = r^T z of iteration it + 1 over r^T z of iteration it (first: p = z)
__global__ void __launch_bounds__(256) k_harm_direction(int64_t n, const double *__restrict__ z, double *__restrict__ p, int64_t ld, DynGate g,
                                                       const double *__restrict__ cs, int first) {
    if (dyn_closed(g)) return;
    Cx beta{0.0, 0.0};
    if (!first) {
        const double *sc = harm_cs(g, cs);
        beta = cdiv(Cx{sc[4], sc[5]}, Cx{sc[0], sc[1]});
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (first) { p[i] = z[i]; p[ld + i] = z[ld + i]; }
        else {
            const Cx bp = cmul(beta, Cx{p[i], p[ld + i]});
            p[i] = z[i] + bp.re;
            p[ld + i] = z[ld + i] + bp.im;
        }
    }
}

// after a converged frequency: partials {|f - Z x|^2}, the probe values {re, im} of x and its row of the fields {re plane, im plane} (null: none)
__global__ void __launch_bounds__(256) k_harm_finish(int64_t n, const double *__restrict__ f, const double *__restrict__ Zx, const double *__restrict__ x,
                                                    int64_t ld, int nProbe, const int64_t *__restrict__ probeVars, double *__restrict__ probeRow,
                                                    double *__restrict__ fieldRow, double *__restrict__ partials) {
    __shared__ double red[8];
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nProbe; j += (int64_t)gridDim.x * 256) {
        probeRow[2 * j] = x[probeVars[j]];
        probeRow[2 * j + 1] = x[ld + probeVars[j]];
    }
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double a = f[i] - Zx[i], b = f[ld + i] - Zx[ld + i];
        acc[0] = fma(a, a, fma(b, b, acc[0]));
        if (fieldRow) { fieldRow[i] = x[i]; fieldRow[n + i] = x[ld + i]; }
    }
    store_partials<1>(acc, red, partials);
}

// y = zK y + zM M x (acc) or zM M x on both planes; the workgroups' x^T y in partials[.][0, 1]. Returns the number of partials. One pass over M
// (k_spmv_kron_cacc) where its LDS fits and twoPass is not set; else two launches of k_spmv_kron_acc into tmp (two planes) and k_harm_combine.
int launch_spmv_kron_cacc(const SpmvArgs &a, bool acc, Cx zK, Cx zM, const double *x, double *y, int64_t ld, int64_t n, double *tmp, double *partials,
                          const DynGate &g, hipStream_t s, int cap, bool twoPass) {
    if (a.nChunk <= 0) return 0;
    if (a.dim != 2 && a.dim != 3) throw mfh::Error(MFH_ERR_UNSUPPORTED, "k_spmv_kron_cacc: 2D / 3D only");
    const size_t lds = ((size_t)2 * a.dim * a.chunkSlots + 16) * sizeof(double);
    cap = std::max(1, std::min(cap, DYN_GRID_CAP));
    if (!twoPass && lds <= HARM_LDS_MAX) {
        const int grid = (int)std::min<int64_t>(a.nChunk, cap);
        with_dim(a.dim, [&](auto D) { with_bool(acc, [&](auto ACC) {
            launch_k(k_spmv_kron_cacc<D(), ACC()>, dim3(grid), dim3(256), lds, s, a, zK, zM, x, y, ld, partials, g);
        }); });
        CHECK_LAUNCH();
        return grid;
    }
    if (!tmp) throw mfh::Error(MFH_ERR_INVALID, "k_harm_combine: no work vector");
    launch_spmv_kron_acc(a, false, 0.0, 1.0, x, tmp, nullptr, g, s, cap);
    launch_spmv_kron_acc(a, false, 0.0, 1.0, x + ld, tmp + ld, nullptr, g, s, cap);
    const int grid = dyn_grid(n, cap);
    with_bool(acc, [&](auto ACC) {
        launch_k(k_harm_combine<ACC()>, dim3(grid), dim3(256), 0, s, n, zK, zM, x, y, (const double *)tmp, ld, a.fixedMask, partials, g);
    });
    CHECK_LAUNCH();
    return grid;
}

}   // namespace
}}   // namespace mfh::k

using namespace mfh;
using namespace mfhi;
using k::Cx;
using k::DynGate;
using k::DYN_NV;

namespace {

struct HarmonicWork : PencilWork {
    DBuf<double> cscal;                        // the complex scalars of the history (the Hermitian r . r, which the gate reads, is in scal; bb[0] = |f|^2)
    double *f, *x, *r, *z, *p, *Ap, *tmp;      // two planes each: re at v, im at v + ld
    Cx zK{0, 0}, zM{0, 0};                     // the pencil of the solve under way
    double jacobiCM = 0;                       // and the K + jacobiCM M its block-Jacobi takes

    // y = zK K x + zM M x on the free variables; dotDst (may be null): {Re, Im} of x^T y
    void pencil(const double *xin, double *y, double *dotDst, const DynGate &g) {
        const bool haveK = zK.re != 0.0 || zK.im != 0.0;
        lap(-1);
        if (haveK) {
            apply_operator(c, masked, xin, y, nullptr);
            apply_operator(c, masked, xin + ld, y + ld, nullptr);
        }
        lap(0);
        const int np = k::launch_spmv_kron_cacc(mass_spmv_args(c, masked), haveK, zK, zM, xin, y, ld, n, tmp, dotDst ? partials.p : nullptr, g, s,
                                                c->dynGridCap, c->harmTwoPass);
        if (dotDst) sum_to(np, g, dotDst, dotDst + 1);
        lap(1);
    }
    template <bool BJ> void launch_init() {
        const int grid = vec_grid(nRows);
        k::with_dim(d, [&](auto D) {
            k::launch_k(k::k_harm_init<D(), BJ>, dim3(grid), dim3(256), 0, s, nRows, (const double *)dinv.p, (const double *)f, (const double *)Ap, r, z, p, ld, partials.p);
        });
        CHECK_LAUNCH();
        sum_to(grid, k::dyn_open(), BJ ? cscal.p : nullptr, BJ ? cscal.p + 1 : nullptr, scal.p + 2);
    }
    template <bool BJ> void launch_update(int it) {
        const int grid = vec_grid(nRows);
        const DynGate g = gate(it);
        k::with_dim(d, [&](auto D) {
            k::launch_k(k::k_harm_update<D(), BJ>, dim3(grid), dim3(256), 0, s, nRows, (const double *)dinv.p, (const double *)Ap, (const double *)p, x, r, z, ld, g,
                        (const double *)cscal.p, partials.p);
        });
        CHECK_LAUNCH();
        double *const cn = cscal.p + (size_t)(it + 1) * 4;
        sum_to(grid, g, BJ ? cn : nullptr, BJ ? cn + 1 : nullptr, scal.p + (size_t)(it + 1) * 4 + 2);
    }
    // z = B r on both planes with the hierarchy of K, then r^T z of iteration it + 1
    void coarse_precond(int it) {
        const DynGate g = it >= 0 ? gate(it) : k::dyn_open();
        for (int plane = 0; plane < 2; ++plane) {
            const double *rp = r + plane * ld;
            double *zp = z + plane * ld;
            if (useMG) mg_precond(c, rp, zp, it >= 0 ? scal.p : nullptr, it, it >= 0 ? stop : nullptr);
            else tl_precond(c, rp, zp, nullptr, -1);
        }
        const int grid = vec_grid(n);
        hipLaunchKernelGGL(k::k_harm_rz, dim3(grid), dim3(256), 0, s, n, (const double *)r, z, ld, mask, g, partials.p);
        CHECK_LAUNCH();
        double *const cn = cscal.p + (size_t)(it + 1) * 4;
        sum_to(grid, g, cn, cn + 1);
    }
    void direction(int it, bool first) {
        hipLaunchKernelGGL(k::k_harm_direction, dim3(vec_grid(n)), dim3(256), 0, s, n, (const double *)z, p, ld, first ? k::dyn_open() : gate(it), (const double *)cscal.p,
                           first ? 1 : 0);
        CHECK_LAUNCH();
    }

    // the two halves of a COCG solve that pencil_loop calls: r = f - Z x with the first z and p, and iteration `it`
    void start(bool jacobi) {
        MFH_HIP(hipMemsetAsync(cscal.p, 0, cscal.n * sizeof(double), s));
        if (jacobi) ensure_dinv(1.0, jacobiCM);
        pencil(x, Ap, nullptr, k::dyn_open());
        if (jacobi) launch_init<true>();
        else { launch_init<false>(); coarse_precond(-1); direction(-1, true); }
    }
    void iterate(int it, bool jacobi) {
        pencil(p, Ap, cscal.p + (size_t)it * 4 + 2, gate(it));
        if (jacobi) { launch_update<true>(it); lap(2); }
        else { launch_update<false>(it); lap(2); coarse_precond(it); lap(3); }
        direction(it, false);
        lap(4);
    }
    // COCG on Z = zK K + zM M: the right-hand side in f with the threshold in stop[0], the start vector in x. Returns the iterations taken,
    // -1: maxit reached (x then holds the last iterate), -2: breakdown (a residual norm is not finite). restart: a continuation from the true
    // residual of a converged iterate (a few iterations: short batches, and the guess for the next frequency stays).
    // Batches: the first read-back comes after as many iterations as the previous frequency took; where that was not enough the next ones come in
    // short batches: an iteration past convergence still pays for its two (ungated) K products, ten times what a read-back costs.
    int solve(Cx zK, Cx zM, bool jacobi, double jacobiCM, bool restart) {
        this->zK = zK; this->zM = zM; this->jacobiCM = jacobiCM;
        return pencil_loop(*this, jacobi, restart ? short_batch() : batch, [&] { return short_batch(); }, !restart);
    }
    // |f|^2 of the load in this->f -> bb[0] and the threshold rtol^2 |f|^2 -> stop[0]
    void set_threshold(double rtol) {
        const int grid = vec_grid(n);
        hipLaunchKernelGGL(k::k_harm_norm2, dim3(grid), dim3(256), 0, s, n, (const double *)f, ld, partials.p);
        CHECK_LAUNCH();
        const int col[2] = {0, 0};
        const double sc[2] = {rtol * rtol, 1.0};
        double *const dst[2] = {stop, bb};
        reduce(grid, 2, col, sc, dst, k::dyn_open());
    }
};

// What mfh_harmonic and the test hook of its loop (mfh_debug_harmonic_cocg) share: setup_pencil_work, the work vectors and the complex history of
// HarmonicWork::solve. Returns whether the loop runs block-Jacobi.
bool setup_harmonic_work(mfh_ctx *c, HarmonicWork &w, const char *who, int maxit) {
    const bool jacobi = setup_pencil_work(c, w, who, maxit);
    w.vec.alloc((size_t)w.ld * 14);
    w.vec.zero(w.s);
    double *q = w.vec.p;
    double **slots[7] = {&w.f, &w.x, &w.r, &w.z, &w.p, &w.Ap, &w.tmp};
    for (auto sl : slots) { *sl = q; q += 2 * w.ld; }
    w.cscal.alloc(((size_t)maxit + 2) * 4);
    return jacobi;
}

void check_params(const mfh_ctx *c, const mfh_harmonic_params *p, const double *omega, const double *fRe, const int64_t *probeVars, int32_t nProbe,
                  const double *probeOut) {
    require(p != nullptr, MFH_ERR_INVALID, "mfh_harmonic: params is null");
    require(p->nFreq >= 0 && p->maxit > 0, MFH_ERR_INVALID, "mfh_harmonic: nFreq >= 0, maxit > 0");
    require(p->density > 0.0 && std::isfinite(p->density), MFH_ERR_INVALID, "mfh_harmonic: density > 0");
    require(p->rayleighMass >= 0.0 && p->rayleighStiff >= 0.0 && std::isfinite(p->rayleighMass) && std::isfinite(p->rayleighStiff), MFH_ERR_INVALID,
            "mfh_harmonic: the Rayleigh coefficients are not negative");
    require(p->lossFactor >= 0.0 && std::isfinite(p->lossFactor), MFH_ERR_INVALID, "mfh_harmonic: the loss factor is not negative");
    require(p->rtol > 0.0 && p->rtol < 1.0, MFH_ERR_INVALID, "mfh_harmonic: 0 < rtol < 1");
    require((p->flags & ~MFH_HARM_WARM_START) == 0, MFH_ERR_INVALID, "mfh_harmonic: unknown flag");
    require(p->nFreq == 0 || omega != nullptr, MFH_ERR_INVALID, "mfh_harmonic: omega is null");
    require(fRe != nullptr, MFH_ERR_INVALID, "mfh_harmonic: fRe is null");
    for (int32_t k2 = 0; k2 < p->nFreq; ++k2) {
        require(std::isfinite(omega[k2]) && omega[k2] >= 0.0, MFH_ERR_INVALID, "mfh_harmonic: a frequency is negative or not finite");
        require(omega[k2] > 0.0 || !c->fixedVars.empty(), MFH_ERR_INVALID, "mfh_harmonic: omega = 0 needs fixed variables (K alone is singular)");
    }
    require(nProbe >= 0 && (nProbe == 0 || (probeVars && probeOut)), MFH_ERR_INVALID, "mfh_harmonic: probes need their variables and their output");
    const int64_t nv = (int64_t)c->bs() * c->nDoF;
    for (int32_t j = 0; j < nProbe; ++j) require(probeVars[j] >= 0 && probeVars[j] < nv, MFH_ERR_INVALID, "mfh_harmonic: probe variable out of range");
}

}   // namespace

namespace mfhi {
void harmonic_product(mfh_ctx *c, bool masked, const double *zK, const double *zM, const double *x, double *y, int64_t ld, double *tmp) {
    const int64_t n = (int64_t)c->bs() * c->nDoF;
    const bool haveK = zK[0] != 0.0 || zK[1] != 0.0;
    if (haveK) { apply_operator(c, masked, x, y, nullptr); apply_operator(c, masked, x + ld, y + ld, nullptr); }
    k::launch_spmv_kron_cacc(mass_spmv_args(c, masked), haveK, Cx{zK[0], zK[1]}, Cx{zM[0], zM[1]}, x, y, ld, n, tmp, nullptr, k::dyn_open(), c->stream,
                             c->dynGridCap, c->harmTwoPass);
}
}   // namespace mfhi

extern "C" {

mfh_status mfh_harmonic(mfh_ctx *c, const mfh_harmonic_params *prm, const double *omega, const double *fRe, const double *fIm, const int64_t *probeVars,
                        int32_t nProbe, double *probeOut, double *fields, int32_t *iterations, double *trueResiduals, mfh_harmonic_info *info) {
    if (info) { *info = mfh_harmonic_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_harmonic: null context");
    check_params(c, prm, omega, fRe, probeVars, nProbe, probeOut);
    const mfh_harmonic_params P = *prm;
    prepare_pencil(c, "mfh_harmonic");
    hipStream_t s = c->stream;
    c->harmNote.clear();
    auto note = [&](const std::string &t) { if (!c->harmNote.empty()) c->harmNote += "; "; c->harmNote += t; };
    WideGuard guard(c);
    if (guard.widened) note("the pattern held the upper triangle only: symbolic phase re-run with both triangles (what option matrix_storage 0 does) for this call");
    EventTimer tsetup(s);
    const bool masked = !c->fixedVars.empty();
    HarmonicWork w;
    const bool jacobi = setup_harmonic_work(c, w, "mfh_harmonic", P.maxit);
    if (w.wantCoarse && !masked) note("no fixed variables (K singular): block-Jacobi of K + w^2 density M in place of the two-level / multigrid preconditioner");
    else if (w.wantCoarse && jacobi) note(c->precondNote.empty() ? std::string("two-level / multigrid preconditioner unavailable: block-Jacobi of K + w^2 density M") : c->precondNote + " (block-Jacobi of K + w^2 density M)");
    else if (!w.wantCoarse) note("block-Jacobi of K + w^2 density M on both planes");
    else if (w.useTL && c->precond == MFH_PRECOND_MULTIGRID) note(c->precondNote.empty() ? std::string("multigrid hierarchy unavailable: two-level preconditioner of K on both planes") : c->precondNote);
    else note(w.useMG ? "multigrid V-cycle of K on both planes" : "two-level preconditioner of K on both planes");
    if (c->harmTwoPass) note("mass product: two real passes and a combine kernel (option harmonic_two_pass)");
    const int64_t ld = w.ld;

    const int nFreq = P.nFreq;
    const int64_t rowLen = 2 * w.n;
    // field rows wait on the device and leave in groups (256 MB at most, one row at least)
    const int64_t fieldCap = fields ? std::max<int64_t>(1, std::min<int64_t>(std::max(nFreq, 1), ((int64_t)1 << 25) / std::max<int64_t>(rowLen, 1))) : 0;
    DBuf<double> dField, dProbe, dRes;
    DBuf<int64_t> dProbeVars;
    if (fields) dField.alloc((size_t)fieldCap * (size_t)rowLen);
    if (nProbe) {
        dProbe.alloc((size_t)std::max(nFreq, 1) * (size_t)nProbe * 2);
        dProbeVars.alloc((size_t)nProbe);
        MFH_HIP(hipMemcpyAsync(dProbeVars.p, probeVars, (size_t)nProbe * sizeof(int64_t), hipMemcpyHostToDevice, s));
    }
    dRes.alloc((size_t)std::max(nFreq, 1));
    dRes.zero(s);
    upload(w.f, fRe, w.n, s);
    if (fIm) upload(w.f + ld, fIm, w.n, s);
    if (masked) { k::launch_mask(w.n, w.mask, w.f, s); k::launch_mask(w.n, w.mask, w.f + ld, s); }
    double hbb = 0.0;
    w.set_threshold(P.rtol);            // the same for every frequency
    MFH_HIP(hipMemcpyAsync(&hbb, w.bb, sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    require(std::isfinite(hbb), MFH_ERR_INVALID, "mfh_harmonic: the load has an entry that is not finite");
    const double setupMs = tsetup.stop();

    EventTimer tsolve(s);
    int freqsDone = 0, itTotal = 0, itMax = 0, restarts = 0;
    int64_t held = 0, written = 0;
    auto flush_fields = [&]() {
        if (held) MFH_HIP(hipMemcpyAsync(fields + (size_t)written * (size_t)rowLen, dField.p, (size_t)held * (size_t)rowLen * sizeof(double), hipMemcpyDeviceToHost, s));
        MFH_HIP(hipStreamSynchronize(s));
        written += held;
        held = 0;
    };
    mfh_status failure = MFH_OK;
    std::string failText;
    if (hbb == 0.0) {                   // f^ = 0 on the free variables: u^ = 0 at every frequency, no iteration
        if (fields) std::fill(fields, fields + (size_t)nFreq * (size_t)rowLen, 0.0);
        if (nProbe) std::fill(probeOut, probeOut + (size_t)nFreq * (size_t)nProbe * 2, 0.0);
        for (int k2 = 0; k2 < nFreq; ++k2) { if (iterations) iterations[k2] = 0; if (trueResiduals) trueResiduals[k2] = 0.0; }
        freqsDone = nFreq;
        note("zero load: zero response");
    } else {
        const bool warm = (P.flags & MFH_HARM_WARM_START) != 0;
        for (int k2 = 0; k2 < nFreq; ++k2) {
            const double om = omega[k2];
            const Cx zK{1.0, P.lossFactor + om * P.rayleighStiff};
            const Cx zM{-P.density * om * om, P.density * om * P.rayleighMass};
            if (!warm && k2 > 0) MFH_HIP(hipMemsetAsync(w.x, 0, (size_t)ld * 2 * sizeof(double), s));
            // The recurrence's residual drifts on undamped, indefinite systems (small p^T Z p): the true residual comes from one more pencil product,
            // with the probe values and the field row. Where it is more than 10 x the threshold the COCG continues from that true residual (solve
            // recomputes r = f - Z x), twice at the most; the iterations add up.
            double *fieldRow = nullptr;
            if (fields) {
                if (held == fieldCap) flush_fields();
                fieldRow = dField.p + (size_t)held * (size_t)rowLen;
                ++held;
            }
            int its = 0, itsFreq = 0;
            for (int attempt = 0; attempt < 3; ++attempt) {
                its = w.solve(zK, zM, jacobi, om * om * P.density, attempt > 0);
                if (its < 0) break;
                itsFreq += its;
                if (attempt > 0) ++restarts;
                w.pencil(w.x, w.Ap, nullptr, k::dyn_open());      // (the pencil of the solve)
                const int grid = w.vec_grid(w.n);
                hipLaunchKernelGGL(k::k_harm_finish, dim3(grid), dim3(256), 0, s, w.n, (const double *)w.f, (const double *)w.Ap, (const double *)w.x, ld, (int)nProbe,
                                   (const int64_t *)dProbeVars.p, nProbe ? dProbe.p + (size_t)k2 * (size_t)nProbe * 2 : nullptr, fieldRow, w.partials.p);
                CHECK_LAUNCH();
                w.sum_to(grid, k::dyn_open(), dRes.p + k2);
                double hr = 0.0;
                MFH_HIP(hipMemcpyAsync(&hr, dRes.p + k2, sizeof(double), hipMemcpyDeviceToHost, s));
                MFH_HIP(hipStreamSynchronize(s));
                if (!std::isfinite(hr)) { its = -2; break; }
                if (hr <= 100.0 * P.rtol * P.rtol * hbb) break;
            }
            if (its < 0) {
                failure = MFH_ERR_NOT_CONVERGED;
                failText = its == -1 ? "mfh_harmonic: the COCG of frequency " + std::to_string(k2) + " reached maxit" : "mfh_harmonic: COCG breakdown at frequency " + std::to_string(k2) + " (a residual norm is not finite)";
                if (fields) --held;                 // (its row is not written out)
                break;
            }
            if (iterations) iterations[k2] = itsFreq;
            itTotal += itsFreq;
            itMax = std::max(itMax, itsFreq);
            freqsDone = k2 + 1;
        }
        if (fields) flush_fields();
        if (restarts) note("recurrence drift: " + std::to_string(restarts) + " continuation(s) from the true residual");
        std::vector<double> hres((size_t)std::max(freqsDone, 1));
        if (freqsDone) {
            if (nProbe) MFH_HIP(hipMemcpyAsync(probeOut, dProbe.p, (size_t)freqsDone * (size_t)nProbe * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
            MFH_HIP(hipMemcpyAsync(hres.data(), dRes.p, (size_t)freqsDone * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        MFH_HIP(hipStreamSynchronize(s));
        double worst = 0.0;
        for (int k2 = 0; k2 < freqsDone; ++k2) {
            const double t = std::sqrt(hres[(size_t)k2] / hbb);
            if (trueResiduals) trueResiduals[k2] = t;
            worst = std::isfinite(t) ? std::max(worst, t) : t;
        }
        if (info) info->worstTrueResidual = worst;
    }
    const double solveMs = tsolve.stop();
    if (w.timing)
        fprintf(stderr, "[mfh_harmonic] n %lld frequencies %d iterations %d | ms: K %.3f M %.3f update %.3f precond %.3f direction %.3f readback %.3f\n",
                (long long)w.n, freqsDone, itTotal, w.tPhase[0], w.tPhase[1], w.tPhase[2], w.tPhase[3], w.tPhase[4], w.tPhase[5]);
    if (info) {
        info->freqsDone = freqsDone;
        info->iterationsTotal = itTotal;
        info->iterationsMax = itMax;
        info->precondUsed = w.useMG ? MFH_PRECOND_MULTIGRID : (w.useTL ? MFH_PRECOND_TWO_LEVEL : MFH_PRECOND_BLOCK_JACOBI);
        info->setupMs = setupMs; info->solveMs = solveMs;
        info->note = c->harmNote.c_str();
    }
    if (failure != MFH_OK) throw Error(failure, failText);
    MFH_CATCH(c)
}

// ---- test hook (include/meshfem_hip_extras.h): y^ = Z x^ on the context's operators, dot = {Re, Im} of x^T y
mfh_status mfh_debug_harmonic_apply(mfh_ctx *c, double zKre, double zKim, double zMre, double zMim, int32_t masked, const double *xRe, const double *xIm,
                                    double *yRe, double *yIm, double *dot) {
    MFH_TRY(c)
    require(c && xRe && xIm && yRe && yIm && std::isfinite(zKre) && std::isfinite(zKim) && std::isfinite(zMre) && std::isfinite(zMim), MFH_ERR_INVALID,
            "mfh_debug_harmonic_apply: arguments");
    prepare_pencil(c, "mfh_debug_harmonic_apply");
    hipStream_t s = c->stream;
    WideGuard guard(c);
    prepare_pencil_state(c, "mfh_debug_harmonic_apply", false);
    const int64_t n = (int64_t)c->bs() * c->nDoF, ld = (n + 31) / 32 * 32;
    const bool m = masked != 0 && !c->fixedVars.empty();
    DBuf<double> v, part;
    v.alloc((size_t)ld * 6 + 2); part.alloc((size_t)k::DYN_GRID_CAP * DYN_NV);
    v.zero(s);
    double *dx = v.p, *dy = v.p + 2 * ld, *dt = v.p + 4 * ld, *dd = v.p + 6 * ld;
    upload(dx, xRe, n, s);
    upload(dx + ld, xIm, n, s);
    const Cx zK{zKre, zKim}, zM{zMre, zMim};
    const bool haveK = zKre != 0.0 || zKim != 0.0;
    if (haveK) { apply_operator(c, m, dx, dy, nullptr); apply_operator(c, m, dx + ld, dy + ld, nullptr); }
    const int np = k::launch_spmv_kron_cacc(mass_spmv_args(c, m), haveK, zK, zM, dx, dy, ld, n, dt, part.p, k::dyn_open(), s, c->dynGridCap, c->harmTwoPass);
    k::launch_sum(np, part.p, k::dyn_open(), s, dd, dd + 1);
    MFH_HIP(hipMemcpyAsync(yRe, dy, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(yIm, dy + ld, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (dot) MFH_HIP(hipMemcpyAsync(dot, dd, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

// HarmonicWork::solve (restart = false) on (f^, x0^) as a frequency of mfh_harmonic calls it: the load masked and its threshold set the same way
mfh_status mfh_debug_harmonic_cocg(mfh_ctx *c, const double *zK, const double *zM, double jacobiCM, double rtol, int32_t maxit, const double *fRe, const double *fIm,
                                   const double *x0Re, const double *x0Im, double *xRe, double *xIm, double *history, double *chistory, int32_t *its) {
    MFH_TRY(c)
    require(c && zK && zM && fRe && xRe && xIm && history && chistory && its && std::isfinite(jacobiCM) && rtol > 0.0 && rtol < 1.0 && maxit > 0, MFH_ERR_INVALID,
            "mfh_debug_harmonic_cocg: arguments");
    require(std::isfinite(zK[0]) && std::isfinite(zK[1]) && std::isfinite(zM[0]) && std::isfinite(zM[1]), MFH_ERR_INVALID, "mfh_debug_harmonic_cocg: coefficients");
    prepare_pencil(c, "mfh_debug_harmonic_cocg");
    hipStream_t s = c->stream;
    WideGuard guard(c);
    HarmonicWork w;
    const bool jacobi = setup_harmonic_work(c, w, "mfh_debug_harmonic_cocg", maxit);
    const int64_t ld = w.ld;
    upload(w.f, fRe, w.n, s);
    if (fIm) upload(w.f + ld, fIm, w.n, s);
    if (w.masked) { k::launch_mask(w.n, w.mask, w.f, s); k::launch_mask(w.n, w.mask, w.f + ld, s); }
    w.set_threshold(rtol);
    if (x0Re) upload(w.x, x0Re, w.n, s);       // (zero on the fixed variables, as a converged frequency leaves the warm start)
    if (x0Im) upload(w.x + ld, x0Im, w.n, s);
    const int ret = w.solve(Cx{zK[0], zK[1]}, Cx{zM[0], zM[1]}, jacobi, jacobiCM, false);
    MFH_HIP(hipMemcpyAsync(xRe, w.x, (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(xIm, w.x + ld, (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(history, w.scal.p, ((size_t)maxit + 1) * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(chistory, w.cscal.p, ((size_t)maxit + 1) * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    *its = ret;
    if (ret < 0) throw Error(MFH_ERR_NOT_CONVERGED, ret == -1 ? "mfh_debug_harmonic_cocg: the COCG reached maxit" : "mfh_debug_harmonic_cocg: COCG breakdown");
    MFH_CATCH(c)
}

}   // extern "C"
