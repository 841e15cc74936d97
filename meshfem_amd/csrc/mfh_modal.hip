// Modal superposition (mfh_modal_set_basis, mfh_modal_coordinates, mfh_modal_harmonic, include/meshfem_hip.h; docs/design/04_21_modal_superposition.md):
// frequency sweeps on a mode basis that stays on the device. With M-orthonormal eigenpairs (lambda_j, phi_j) of (K, density M) the response of
// mfh_harmonic's system Z(w) u^ = f^ is
//     u^(w) = sum_j phi_j q_j(w) + r_s / zK(w),   q_j = g_j / d_j,   g = Phi^T f^,
//     d_j = lambda_j zK - w^2 + i w aR + 2 i zeta_j sqrt(lambda_j) w,   zK = 1 + i (eta + w bR),
// r_s = u_s - sum_j phi_j g_j / lambda_j the static correction with K u_s = f^ (optional). The nModes x nFreq scalars d_j, q_j are formed on the host in
// double precision; the device holds B = [Phi | r_re | r_im] (columns ld apart, the layout of the deflation set of mfh_modes.hip) and expands.
//   k_modal_expand<NP>  out[p][row] = sum_j B_j[row] C[j][p]: the lanes own the rows, a lane keeps the NP sums of its row in registers and streams the
//                       nb <= 258 columns of B once (four loads in flight); C is wave-uniform and read-only, so its entries come through scalar loads
//                       (as in k_deflate_update). The value of (row, plane) is the fma chain over j ascending from +0: its bits depend neither on
//                       NP, nor on how the planes are grouped into passes, nor on the grid -- the probes (the same kernel on the gathered probe rows
//                       of B) equal the field entries bit for bit. Plain vector stores, no LDS, no atomics.
//   k_modal_gram        partials of A^T V for na <= 258 columns of A against nv <= 8 columns of V, a tile of 8 x 8 column pairs per workgroup;
//   k_modal_gram_sum    adds the workgroups' partials in workgroup order: G = Phi^T (density M Phi), g = Phi^T [f_re f_im], q = Phi^T (density M u).
//                       Ordered two-stage sums, no floating-point atomics; the row partition depends on n only.
// The mass products are k_spmv_kron_acc's (mfh_pencil.hh), the true residual's operator product mfh_harmonic's own (harmonic_product, mfh_harmonic.hip).
// The same basis serves load histories (mfh_modal_transient; docs/design/04_22_modal_transient.md): k_modal_slope, k_modal_march, k_modal_series
// below, the step coefficients from mfh_modal_coeffs.cpp.
// The three drivers set their loads up through one path (ModalLoads): the static solves, the masked loads on the device, g and the correction columns.
// And quadratic forms per row, phi_i^T C phi_i, for random vibration and response spectra (mfh_modal_quadratic, mfh_modal_random;
// docs/design/04_23_modal_random.md): k_modal_sumsq below on the factor C = F F^T that mfh_modal_cov.cpp forms on the host.
#include "mfh_pencil.hh"
#include <chrono>
#include <functional>
#include <optional>

namespace mfh { namespace k {

namespace {

constexpr int MODAL_MAXM = 256;         // modes of a basis
constexpr int MODAL_MAXB = MODAL_MAXM + 2;   // ... and the two static-correction columns behind them
constexpr int MODAL_NP = 32;            // planes per pass of k_modal_expand by default: the cheapest per plane of {8, 16, 32} (profiles/r18_modal.md); a pass
                                        // with fewer planes left takes the smallest instantiation that holds them
constexpr int MODAL_NP_MAX = 32;
constexpr int MODAL_GRID_CAP = 2048;    // workgroups of k_modal_expand
constexpr int MG_TA = 8, MG_TV = 8;     // column-pair tile of a workgroup of k_modal_gram
constexpr int MG_GRID_CAP = 256;        // its workgroups along the rows (= partials the second stage adds per entry)

// out[(p0 + t) planeStride + row] = sum_j B[j ldb + row] C[j ldc + p0 + t] for t < np <= NP. C: nb rows of ldc doubles, zero-padded to p0 + NP.
template <int NP>
__global__ void __launch_bounds__(256) k_modal_expand(int64_t n, const double *__restrict__ B, int64_t ldb, int nb, const double *__restrict__ C, int ldc, int p0,
                                                     int np, double *__restrict__ out, int64_t planeStride) {
    const double *c0 = C + p0;
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n; row += (int64_t)gridDim.x * 256) {
        double s[NP];
#pragma unroll
        for (int t = 0; t < NP; ++t) s[t] = 0.0;
        const double *b = B + row;
        int j = 0;
        for (; j + 4 <= nb; j += 4) {
            const double b0 = b[(int64_t)j * ldb], b1 = b[(int64_t)(j + 1) * ldb], b2 = b[(int64_t)(j + 2) * ldb], b3 = b[(int64_t)(j + 3) * ldb];
            const double *c = c0 + (int64_t)j * ldc;
#pragma unroll
            for (int t = 0; t < NP; ++t) s[t] = fma(b0, c[t], s[t]);
#pragma unroll
            for (int t = 0; t < NP; ++t) s[t] = fma(b1, c[ldc + t], s[t]);
#pragma unroll
            for (int t = 0; t < NP; ++t) s[t] = fma(b2, c[2 * ldc + t], s[t]);
#pragma unroll
            for (int t = 0; t < NP; ++t) s[t] = fma(b3, c[3 * ldc + t], s[t]);
        }
        for (; j < nb; ++j) {
            const double b0 = b[(int64_t)j * ldb];
            const double *c = c0 + (int64_t)j * ldc;
#pragma unroll
            for (int t = 0; t < NP; ++t) s[t] = fma(b0, c[t], s[t]);
        }
#pragma unroll
        for (int t = 0; t < NP; ++t)
            if (t < np) out[(int64_t)(p0 + t) * planeStride + row] = s[t];
    }
}

// partials[(blockIdx.y na + i) nv + j] = sum over the rows of this workgroup of A_i V_j, i in the workgroup's tile of MG_TA columns of A. Columns
// past the end are clamped to the last one (their sums are not written): the loop carries no branch.
__global__ void __launch_bounds__(256) k_modal_gram(int64_t n, const double *__restrict__ A, int64_t lda, int na, const double *__restrict__ V, int64_t ldv, int nv,
                                                   double *__restrict__ partials) {
    __shared__ double red[4][MG_TA * MG_TV];
    const int a0 = blockIdx.x * MG_TA;
    const double *pa[MG_TA], *pv[MG_TV];
#pragma unroll
    for (int i = 0; i < MG_TA; ++i) pa[i] = A + (int64_t)min(a0 + i, na - 1) * lda;
#pragma unroll
    for (int j = 0; j < MG_TV; ++j) pv[j] = V + (int64_t)min(j, nv - 1) * ldv;
    double acc[MG_TA][MG_TV];
#pragma unroll
    for (int i = 0; i < MG_TA; ++i)
#pragma unroll
        for (int j = 0; j < MG_TV; ++j) acc[i][j] = 0.0;
    for (int64_t row = (int64_t)blockIdx.y * 256 + threadIdx.x; row < n; row += (int64_t)gridDim.y * 256) {
        double a[MG_TA], v[MG_TV];
#pragma unroll
        for (int i = 0; i < MG_TA; ++i) a[i] = pa[i][row];
#pragma unroll
        for (int j = 0; j < MG_TV; ++j) v[j] = pv[j][row];
#pragma unroll
        for (int i = 0; i < MG_TA; ++i)
#pragma unroll
            for (int j = 0; j < MG_TV; ++j) acc[i][j] = fma(a[i], v[j], acc[i][j]);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < MG_TA; ++i)
#pragma unroll
        for (int j = 0; j < MG_TV; ++j) {
            const double v = wave_sum(acc[i][j]);
            if (lane == 0) red[w][i * MG_TV + j] = v;
        }
    __syncthreads();
    if (threadIdx.x < MG_TA * MG_TV) {
        const int i = threadIdx.x / MG_TV, j = threadIdx.x - i * MG_TV;
        if (a0 + i < na && j < nv)
            partials[((int64_t)blockIdx.y * na + a0 + i) * nv + j] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    }
}

// G[e] = the partials of entry e added in workgroup order
__global__ void __launch_bounds__(256) k_modal_gram_sum(int nPart, int count, const double *__restrict__ partials, double *__restrict__ G) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    double v = 0.0;
    for (int b = 0; b < nPart; ++b) v += partials[(int64_t)b * count + e];
    G[e] = v;
}

// Bp[j ldp + i] = B[j ldb + vars[i]]: the probe rows of the basis
__global__ void __launch_bounds__(256) k_modal_gather_rows(int nProbe, int nb, const int64_t *__restrict__ vars, const double *__restrict__ B, int64_t ldb,
                                                          double *__restrict__ Bp, int64_t ldp) {
    const int64_t total = (int64_t)nProbe * nb;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t j = t / nProbe, i = t - j * nProbe;
        Bp[j * ldp + i] = B[j * ldb + vars[i]];
    }
}

// partials {|f - y|^2} over both planes (y null: |f|^2)
__global__ void __launch_bounds__(256) k_modal_resnorm(int64_t n, const double *__restrict__ f, const double *__restrict__ y, int64_t ld, double *__restrict__ partials) {
    __shared__ double red[8];
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double a = f[i] - (y ? y[i] : 0.0), b = f[ld + i] - (y ? y[ld + i] : 0.0);
        acc[0] = fma(a, a, fma(b, b, acc[0]));
    }
    store_partials<1>(acc, red, partials);
}

// dst[i] = sign src[i], sign = +-1: a column mfh_modes_many left on the device, with the sign its host copy carries (exact either way)
__global__ void __launch_bounds__(256) k_modal_adopt(int64_t n, const double *__restrict__ src, double sign, double *__restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = sign * src[i];
}

int modal_np_for(int planesPerPass) { return planesPerPass <= 8 ? 8 : (planesPerPass <= 16 ? 16 : 32); }

// out[p planeStride + row] for the planes [0, nPlanes) in passes of planesPerPass (1 .. 32) planes; C: device, nb rows of ldc doubles, zero beyond
// nPlanes up to ldc >= nPlanes + 32
void launch_modal_expand(int64_t n, const double *B, int64_t ldb, int nb, const double *C, int ldc, int nPlanes, int planesPerPass, double *out, int64_t planeStride,
                         hipStream_t s) {
    if (n <= 0 || nPlanes <= 0) return;
    const dim3 grid(grid_for(n, MODAL_GRID_CAP)), block(256);
    for (int p0 = 0; p0 < nPlanes; p0 += planesPerPass) {
        const int np = std::min(planesPerPass, nPlanes - p0);
        with_int<8, 16, 32>(modal_np_for(np), [&](auto NP) { launch_k(k_modal_expand<NP()>, grid, block, 0, s, n, B, ldb, nb, C, ldc, p0, np, out, planeStride); });
    }
    CHECK_LAUNCH();
}

// G (device, na x nv row-major) = A^T V; partials: scratch of MG_GRID_CAP * na * nv doubles
void launch_modal_gram(int64_t n, const double *A, int64_t lda, int na, const double *V, int64_t ldv, int nv, double *partials, double *G, hipStream_t s) {
    const int rows = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, MG_GRID_CAP)), count = na * nv;
    hipLaunchKernelGGL(k_modal_gram, dim3((na + MG_TA - 1) / MG_TA, rows), dim3(256), 0, s, n, A, lda, na, V, ldv, nv, partials);
    hipLaunchKernelGGL(k_modal_gram_sum, dim3((count + 255) / 256), dim3(256), 0, s, rows, count, (const double *)partials, G);
    CHECK_LAUNCH();
}

// ---------------------------------------------------------------- quadratic forms per row (mfh_modal_quadratic, mfh_modal_random; docs/design/04_23_modal_random.md)
// v[row] = phi^T C phi of the row phi of B for C = F F^T, as sum_t s_t^2 with s_t = sum_j B_j[row] F[j][t]: k_modal_expand's streaming loop over the
// columns cols[0 .. nc) (wave-uniform: the list and the coefficients come through scalar loads) with another epilogue,
//     acc = first ? 0.0 : out[row];   acc = fma(s_t, s_t, acc) for t < np ascending;   out[row] = last && root ? sqrt(acc) : acc,
// np <= NP the columns of F this pass takes (the sums beyond them are formed and dropped, as k_modal_expand drops the planes beyond np), so neither
// NP nor the pass boundaries change a bit. F: rows of ldf doubles, readable (zero) up to t0 + NP. A column whose coefficients are all exactly zero in [t0, t0 + NP) may be left out of the list: fma(b, 0, s) = s for finite b.
template <int NP>
__global__ void __launch_bounds__(256) k_modal_sumsq(int64_t n, const double *__restrict__ B, int64_t ldb, const int32_t *__restrict__ cols, int nc,
                                                    const double *__restrict__ F, int ldf, int t0, int np, int first, int root, double *__restrict__ out) {
    const double *f0 = F + t0;
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n; row += (int64_t)gridDim.x * 256) {
        double s[NP];
#pragma unroll
        for (int t = 0; t < NP; ++t) s[t] = 0.0;
        const double *b = B + row;
        int j = 0;
        for (; j + 4 <= nc; j += 4) {
            const int c0 = cols[j], c1 = cols[j + 1], c2 = cols[j + 2], c3 = cols[j + 3];
            const double b0 = b[(int64_t)c0 * ldb], b1 = b[(int64_t)c1 * ldb], b2 = b[(int64_t)c2 * ldb], b3 = b[(int64_t)c3 * ldb];
            const double *f_0 = f0 + (int64_t)c0 * ldf, *f_1 = f0 + (int64_t)c1 * ldf, *f_2 = f0 + (int64_t)c2 * ldf, *f_3 = f0 + (int64_t)c3 * ldf;
#pragma unroll
            for (int t = 0; t < NP; ++t) s[t] = fma(b0, f_0[t], s[t]);
#pragma unroll
            for (int t = 0; t < NP; ++t) s[t] = fma(b1, f_1[t], s[t]);
#pragma unroll
            for (int t = 0; t < NP; ++t) s[t] = fma(b2, f_2[t], s[t]);
#pragma unroll
            for (int t = 0; t < NP; ++t) s[t] = fma(b3, f_3[t], s[t]);
        }
        for (; j < nc; ++j) {
            const int c0 = cols[j];
            const double b0 = b[(int64_t)c0 * ldb];
            const double *f_0 = f0 + (int64_t)c0 * ldf;
#pragma unroll
            for (int t = 0; t < NP; ++t) s[t] = fma(b0, f_0[t], s[t]);
        }
        double acc = first ? 0.0 : out[row];
#pragma unroll
        for (int t = 0; t < NP; ++t)
            if (t < np) acc = fma(s[t], s[t], acc);
        out[row] = root ? sqrt(acc) : acc;
    }
}

// The passes of one matrix, planned on the host. F: nb x rank row-major with the pivots piv (mfh_psd_factor): a pass whose first column is t0 leaves out
// the basis columns piv[0 .. t0), whose coefficients are exactly zero from column t0 on; piv null: every pass streams all nb columns.
struct SumsqPlan {
    int nb = 0, rank = 0, ldf = 0, np = MODAL_NP, passes = 0;
    std::vector<int32_t> cols;          // the lists of the passes, one after the other
    std::vector<int> off, cnt;          // ... where each begins, and its length
    DBuf<double> dF;
    DBuf<int32_t> dCols;
    void build(int nb_, const double *F, int ldFh, int rank_, const int32_t *piv, int planesPerPass, hipStream_t s) {
        nb = nb_; rank = rank_; np = planesPerPass; ldf = rank + MODAL_NP_MAX;
        cols.clear(); off.clear(); cnt.clear(); passes = 0;
        if (rank <= 0) return;
        std::vector<double> hf((size_t)nb * ldf, 0.0);
        for (int j = 0; j < nb; ++j)
            for (int t = 0; t < rank; ++t) hf[(size_t)j * ldf + t] = F[(size_t)j * ldFh + t];
        std::vector<uint8_t> out((size_t)nb, 0);
        int done = 0;
        for (int t0 = 0; t0 < rank; t0 += np) {
            if (piv) for (; done < t0; ++done) out[(size_t)piv[done]] = 1;
            off.push_back((int)cols.size());
            for (int j = 0; j < nb; ++j)
                if (!out[(size_t)j]) cols.push_back(j);
            cnt.push_back((int)cols.size() - off.back());
            ++passes;
        }
        dF.upload(hf, s);
        dCols.upload(cols, s);
    }
    // out[row] = (root ? sqrt : id)(sum_t s_t^2) for the n rows of B (columns ldb apart); rank 0: zeros, B is not read
    // only = -1: every pass; else that pass alone (timing)
    void run(int64_t n, const double *B, int64_t ldb, bool root, double *out, hipStream_t s, int only = -1) const {
        if (n <= 0) return;
        if (rank <= 0) { MFH_HIP(hipMemsetAsync(out, 0, (size_t)n * sizeof(double), s)); return; }
        const dim3 grid(grid_for(n, MODAL_GRID_CAP)), block(256);
        for (int p = 0; p < passes; ++p) {
            if (only >= 0 && p != only) continue;
            const int t0 = p * np, left = std::min(np, rank - t0), first = p == 0 ? 1 : 0, rt = (root && p == passes - 1) ? 1 : 0;
            const int32_t *cl = dCols.p + off[(size_t)p];
            const int nc = cnt[(size_t)p];
            with_int<8, 16, 32>(modal_np_for(left), [&](auto NP) { launch_k(k_modal_sumsq<NP()>, grid, block, 0, s, n, B, ldb, cl, nc, (const double *)dF.p, ldf, t0, left, first, rt, out); });
        }
        CHECK_LAUNCH();
    }
};

// ---------------------------------------------------------------- modal transient response (mfh_modal_transient; docs/design/04_22_modal_transient.md)
// Every mode obeys q'' + c q' + lambda q = g a(t) with a piecewise linear between the steps, for which the step is exact:
//     [q ; v]_{r} = A [q ; v]_{r-1} + g (b0 a_{r-1} + b1 s_r),   s_r = (a_r - a_{r-1}) / dt,
// the eight coefficients {A11, A12, b0q, b1q, A21, A22, b0v, b1v} per mode from mfh_modal_transient_coeffs (host, long double). A run is a sequence of
// ROWS r = 0 .. nSteps (row 0: the start state), taken in chunks of rows:
//   k_modal_slope    s_r for all rows at once (IEEE division, off the sequential path)
//   k_modal_march    one lane per mode, the rows of a chunk in sequence; state in / out through a device buffer
//   k_modal_series   probes and energies of all rows of a chunk: the lanes own the rows, the probe rows of the basis are wave-uniform
// and the snapshots are k_modal_expand's on the compact coefficient matrix the march kernel writes.
constexpr int MT_CHUNK = 4096;          // rows of a chunk by default
constexpr int MT_PB = 8;                // probes a workgroup of k_modal_series holds per lane
constexpr int MT_TR = 256, MT_TJ = 16;  // its tile of Q in LDS: rows x modes, rows MT_TJ + 1 doubles apart (odd: the per-lane walk over j hits 64 different banks)
constexpr int MT_COEF_LD = MODAL_MAXM;  // the coefficient table on the device: coef[k MT_COEF_LD + j], k < 8

__global__ void __launch_bounds__(256) k_modal_slope(int64_t rows, const double *__restrict__ amp, double dt, double *__restrict__ slope) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) slope[r] = r > 0 ? (amp[r] - amp[r - 1]) / dt : 0.0;
}

// The rows [0, count) of a chunk; amp and slope point at the chunk's first row (amp[-1] exists unless first = 1: the chunk that holds row 0, which takes
// no step). The operation order of a step, fixed:
//     pq = g b0q, rq = g b1q, pv = g b0v, rv = g b1v                      (once per launch, rounded products)
//     lq = fma(rq, s, pq a0),  lv = fma(rv, s, pv a0)                      (the load term: no state in it)
//     q+ = fma(A11, q, fma(A12, v, lq)),  v+ = fma(A21, q, fma(A22, v, lv))  (two fma deep per component)
// so the state after a row depends on neither the chunk length nor on where a run was cut. a0 and s are wave-uniform (scalar loads). Writes Q[i ldq + j]
// (and V, if not null), and at the snapshot rows i = snapNext, snapNext + snapStride, ... column p = 0, 1, ... of the compact matrix Cs: rows q_j,
// row m = a_i.
__global__ void __launch_bounds__(256) k_modal_march(int m, const double *__restrict__ coef, const double *__restrict__ g, const double *__restrict__ amp,
                                                    const double *__restrict__ slope, int first, int count, double *__restrict__ state, double *__restrict__ Q,
                                                    double *__restrict__ V, int ldq, int snapNext, int snapStride, double *__restrict__ Cs, int ldcs) {
    const int j = threadIdx.x;
    if (j >= m) return;
    const double A11 = coef[j], A12 = coef[MT_COEF_LD + j], A21 = coef[4 * MT_COEF_LD + j], A22 = coef[5 * MT_COEF_LD + j];
    const double gj = g[j];
    const double pq = gj * coef[2 * MT_COEF_LD + j], rq = gj * coef[3 * MT_COEF_LD + j], pv = gj * coef[6 * MT_COEF_LD + j], rv = gj * coef[7 * MT_COEF_LD + j];
    double q = state[j], v = state[MODAL_MAXM + j];
    int p = 0;
    for (int i = 0; i < count; ++i) {
        if (i >= first) {
            const double a0 = amp[i - 1], s = slope[i];
            const double lq = fma(rq, s, pq * a0), lv = fma(rv, s, pv * a0);
            const double qn = fma(A11, q, fma(A12, v, lq)), vn = fma(A21, q, fma(A22, v, lv));
            q = qn; v = vn;
        }
        Q[(int64_t)i * ldq + j] = q;
        if (V) V[(int64_t)i * ldq + j] = v;
        if (i == snapNext) {
            Cs[(int64_t)j * ldcs + p] = q;
            if (j == 0) Cs[(int64_t)m * ldcs + p] = amp[i];
            ++p;
            snapNext += snapStride;
        }
    }
    state[j] = q;
    state[MODAL_MAXM + j] = v;
}

// Rows [0, count) of a chunk, 256 per workgroup. blockIdx.y < ceil(nProbe / MT_PB): the probes p0 .. p0 + MT_PB - 1,
//     probeOut[r nProbe + p] = sum_j Bp[j ldp + p] Q[r ldq + j]  (+ Bp[m ldp + p] amp[r] if corr)
// as the fma chain over j ascending from +0.0 with the correction column last -- k_modal_expand's chain on the same numbers, so a probe equals the
// snapshot entry of its variable bit for bit. Bp (k_modal_gather_rows' layout, zero-padded to ldp, a multiple of 32) is wave-uniform: scalar loads.
// blockIdx.y == ceil(nProbe / MT_PB) (launched only with energies): energies[3 r] = {1/2 sum v_j^2, 1/2 sum (lambda_j q_j) q_j, amp[r] sum g_j q_j}, each
// an fma chain over j ascending. A tile of 256 rows x 16 modes goes through LDS: the global read runs along j (16 doubles of a row at a time), the
// per-lane walk over j reads addresses 17 doubles apart. No atomics.
__global__ void __launch_bounds__(256) k_modal_series(int m, int count, const double *__restrict__ Q, const double *__restrict__ V, int ldq, const double *__restrict__ Bp,
                                                     int ldp, int nProbe, int corr, const double *__restrict__ amp, const double *__restrict__ lam,
                                                     const double *__restrict__ g, double *__restrict__ probeOut, double *__restrict__ energies) {
    __shared__ double tile[MT_TR * (MT_TJ + 1)];
    const int r0 = blockIdx.x * MT_TR, r = r0 + threadIdx.x;
    const int nGroups = (nProbe + MT_PB - 1) / MT_PB;
    auto load_tile = [&](const double *__restrict__ src, int j0) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < MT_TR * MT_TJ; idx += 256) {
            const int rr = idx / MT_TJ, jj = idx - rr * MT_TJ;
            tile[rr * (MT_TJ + 1) + jj] = (r0 + rr < count && j0 + jj < m) ? src[(int64_t)(r0 + rr) * ldq + j0 + jj] : 0.0;
        }
        __syncthreads();
    };
    const double *mine = tile + threadIdx.x * (MT_TJ + 1);
    if ((int)blockIdx.y < nGroups) {
        const int p0 = blockIdx.y * MT_PB;
        double s[MT_PB];
#pragma unroll
        for (int t = 0; t < MT_PB; ++t) s[t] = 0.0;
        for (int j0 = 0; j0 < m; j0 += MT_TJ) {
            load_tile(Q, j0);
            const int nj = min(MT_TJ, m - j0);
            for (int jj = 0; jj < nj; ++jj) {
                const double qv = mine[jj];
                const double *b = Bp + (int64_t)(j0 + jj) * ldp + p0;
#pragma unroll
                for (int t = 0; t < MT_PB; ++t) s[t] = fma(b[t], qv, s[t]);
            }
        }
        if (corr) {
            const double a = r < count ? amp[r] : 0.0;
            const double *b = Bp + (int64_t)m * ldp + p0;
#pragma unroll
            for (int t = 0; t < MT_PB; ++t) s[t] = fma(b[t], a, s[t]);
        }
        if (r < count) {
#pragma unroll
            for (int t = 0; t < MT_PB; ++t)
                if (p0 + t < nProbe) probeOut[(int64_t)r * nProbe + p0 + t] = s[t];
        }
    } else {
        double ke = 0.0, pe = 0.0, w = 0.0;
        for (int j0 = 0; j0 < m; j0 += MT_TJ) {
            const int nj = min(MT_TJ, m - j0);
            load_tile(Q, j0);
            for (int jj = 0; jj < nj; ++jj) {
                const double qv = mine[jj], lq = lam[j0 + jj] * qv;
                pe = fma(lq, qv, pe);
                w = fma(g[j0 + jj], qv, w);
            }
            load_tile(V, j0);
            for (int jj = 0; jj < nj; ++jj) {
                const double vv = mine[jj];
                ke = fma(vv, vv, ke);
            }
        }
        if (r < count) {
            energies[(int64_t)r * 3] = 0.5 * ke;
            energies[(int64_t)r * 3 + 1] = 0.5 * pe;
            energies[(int64_t)r * 3 + 2] = amp[r] * w;
        }
    }
}

void launch_modal_series(int m, int count, const double *Q, const double *V, int ldq, const double *Bp, int64_t ldp, int nProbe, bool corr, const double *amp,
                         const double *lam, const double *g, double *probeOut, double *energies, hipStream_t s) {
    const int nGroups = (nProbe + MT_PB - 1) / MT_PB, ny = nGroups + (energies ? 1 : 0);
    if (count <= 0 || ny == 0) return;
    hipLaunchKernelGGL(k_modal_series, dim3((count + MT_TR - 1) / MT_TR, ny), dim3(256), 0, s, m, count, Q, V, ldq, Bp, (int)ldp, nProbe, corr ? 1 : 0, amp, lam, g, probeOut,
                       energies);
    CHECK_LAUNCH();
}

}   // namespace
}}   // namespace mfh::k

using namespace mfh;
using namespace mfhi;

namespace {

constexpr int MODAL_GROUP_MAX = 128;        // frequencies of a group at most (256 planes: C stays a few hundred KB)

struct Cplx { double re, im; };
Cplx cdivh(const Cplx &a, const Cplx &b) {
    const double d = b.re * b.re + b.im * b.im;
    return Cplx{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
Cplx crecip(const Cplx &b) { return cdivh(Cplx{1.0, 0.0}, b); }

// The modal denominator d_j(w) = lambda zK - w^2 + i (w aR + 2 zeta_j sqrt(lambda) w) with zK = 1 + i (eta + w bR), and the two reciprocals the sweep and
// the response spectra multiply by. (mfh_modal_cov.cpp forms its own: another translation unit, and its reciprocal is not cdivh's.)
Cplx modal_d(double l, double w, double aR, double bR, double eta, double zetaJ) {
    const Cplx zK{1.0, eta + w * bR};
    return Cplx{l * zK.re - w * w, l * zK.im + w * aR + 2.0 * zetaJ * std::sqrt(l) * w};
}
Cplx modal_dinv(double l, double w, double aR, double bR, double eta, double zetaJ) { return crecip(modal_d(l, w, aR, bR, eta, zetaJ)); }
Cplx inv_zK(double w, double bR, double eta) { return crecip(Cplx{1.0, eta + w * bR}); }

void require_for(bool cond, mfh_status code, const char *who, const char *what) {
    if (!cond) throw Error(code, std::string(who) + ": " + what);
}

// a line of the note a driver hands back in its info
void modal_note(mfh_ctx *c, const std::string &t) {
    if (!c->modalNote.empty()) c->modalNote += "; ";
    c->modalNote += t;
}

// cols packed host columns of n doubles to device columns ld apart
void upload_columns(double *dst, int64_t ld, const double *src, int64_t n, int64_t cols, hipStream_t s) {
    MFH_HIP(hipMemcpy2DAsync(dst, (size_t)ld * sizeof(double), src, (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)cols, hipMemcpyHostToDevice, s));
}

bool all_finite(const double *v, int64_t count) {
    std::vector<uint8_t> bad((size_t)std::max(1, host_threads()) + 1, 0);
    parallel_ranges(count, [&](int64_t b, int64_t e, int t) {
        for (int64_t i = b; i < e; ++i)
            if (!std::isfinite(v[i])) { bad[(size_t)std::min<int64_t>(t, (int64_t)bad.size() - 1)] = 1; break; }
    });
    for (uint8_t b : bad) if (b) return false;
    return true;
}

std::vector<int64_t> sorted_fixed(const mfh_ctx *c) {
    std::vector<int64_t> v(c->fixedVars);
    std::sort(v.begin(), v.end());
    return v;
}

// a basis is set and belongs to the state in force
void require_basis(const mfh_ctx *c, const char *who) {
    const mfh_ctx::ModalBasis &mb = c->modal;
    if (mb.nModes <= 0 || !mb.B.p) throw Error(MFH_ERR_STATE, std::string(who) + ": no mode basis (mfh_modal_set_basis)");
    if (!(c->geoValid && mb.geoGen == c->geoGen && mb.densityGen == c->densityGen && mb.n == (int64_t)c->bs() * c->nDoF))
        throw Error(MFH_ERR_STATE, std::string(who) + ": the mode basis is stale (vertex positions, material, density field or DoF map changed since mfh_modal_set_basis)");
    if (sorted_fixed(c) != mb.fixedSet)
        throw Error(MFH_ERR_STATE, std::string(who) + ": the mode basis is stale (the set of fixed variables changed since mfh_modal_set_basis)");
}

// G (host, na x nCols row-major) = A^T (scale M V) for nCols vectors V (device, ldv apart) in batches of MG_TV columns through k_spmv_kron_acc and
// the Gram kernel; scale == 0: G = A^T V, no mass product
void gram_against(mfh_ctx *c, const double *A, int64_t ld, int na, const double *V, int64_t ldv, int nCols, double scale, double *G) {
    hipStream_t s = c->stream;
    const int64_t n = (int64_t)c->bs() * c->nDoF;
    DBuf<double> mv, part, g;
    if (scale != 0.0) { mv.alloc((size_t)ld * k::MG_TV); mv.zero(s); }
    part.alloc((size_t)k::MG_GRID_CAP * na * k::MG_TV);
    g.alloc((size_t)na * k::MG_TV);
    std::vector<double> hg((size_t)na * k::MG_TV);
    for (int c0 = 0; c0 < nCols; c0 += k::MG_TV) {
        const int nv = std::min(k::MG_TV, nCols - c0);
        const double *v = V + (int64_t)c0 * ldv;
        int64_t lv = ldv;
        if (scale != 0.0) {
            for (int j = 0; j < nv; ++j) k::launch_spmv_kron_acc(mass_spmv_args(c, false), false, 0.0, scale, v + (int64_t)j * ldv, mv.p + (int64_t)j * ld, nullptr, k::dyn_open(), s, c->dynGridCap);
            v = mv.p; lv = ld;
        }
        k::launch_modal_gram(n, A, ld, na, v, lv, nv, part.p, g.p, s);
        g.download(hg.data(), (size_t)na * nv, s);
        for (int i = 0; i < na; ++i)
            for (int j = 0; j < nv; ++j) G[(size_t)i * nCols + c0 + j] = hg[(size_t)i * nv + j];
    }
}

// The static solves of the correction (ModalLoads::solve below): K u = f[a] with the
// context's solver and preconditioner for every a < na whose load is not zero off the fixed variables, the fixed variables held at ZERO whatever values
// mfh_solve would hold them at. The counts go to the caller's info as they grow, so that a failed call reports what was done.
void correction_solves(mfh_ctx *c, const char *who, int na, const double *const f[2], const bool nonZero[2], std::vector<double> us[2], double rtol, int maxit,
                       int &staticSolves, int &staticIts, int32_t *infoSolves, int32_t *infoIts) {
    if (!(nonZero[0] || nonZero[1])) return;
    ensure_precond(c);
    ensure_coarse_levels(c, 1);
    if (c->sym.nRows != c->sym.nCols) throw Error(MFH_ERR_UNSUPPORTED, std::string(who) + ": unpartitioned contexts only");
    require_basis(c, who);
    const int64_t n = c->modal.n;
    for (int a = 0; a < na; ++a) {
        if (!nonZero[a]) continue;
        us[a].resize((size_t)n);
        mfh_solve_info li{};
        const bool savedHom = c->solveHomogeneous;
        c->solveHomogeneous = c->anyFixedNonzero;
        try { solve_one(c, f[a], us[a].data(), rtol, maxit, &li); }
        catch (...) { c->solveHomogeneous = savedHom; throw; }
        c->solveHomogeneous = savedHom;
        ++staticSolves;
        staticIts += li.iterations;
        if (infoSolves) *infoSolves = staticSolves;
        if (infoIts) *infoIts = staticIts;
        if (!li.converged) throw Error(MFH_ERR_NOT_CONVERGED, std::string(who) + ": the static solve of the correction did not reach rtol within maxit iterations");
    }
}

// r_a = u_a - sum_j phi_j g_ja / lambda_j for a < na <= 2 into the two reserved columns of B (the other one zero), through the expansion kernel
// itself; g[j na + a]. dC, dTmp: the caller's buffers (they outlive the launches).
void correction_columns(mfh_ctx *c, double *B, int64_t n, int64_t ld, int m, int na, const std::vector<double> us[2], const bool nonZero[2], const double *g,
                        const double *lam, DBuf<double> &dC, DBuf<double> &dTmp, hipStream_t s) {
    MFH_HIP(hipMemsetAsync(B + (int64_t)m * ld, 0, (size_t)ld * 2 * sizeof(double), s));
    for (int a = 0; a < na; ++a)
        if (nonZero[a]) {
            upload(B + (int64_t)(m + a) * ld, us[a].data(), n, s);
            k::launch_mask(n, c->dFixedMask.p, B + (int64_t)(m + a) * ld, s);
        }
    const int ldc = 64;
    std::vector<double> hc((size_t)(m + 2) * ldc, 0.0);
    for (int j = 0; j < m; ++j)
        for (int a = 0; a < na; ++a) hc[(size_t)j * ldc + a] = nonZero[a] ? -(g[(size_t)j * na + a] / lam[(size_t)j]) : 0.0;
    hc[(size_t)m * ldc + 0] = 1.0;
    hc[(size_t)(m + 1) * ldc + 1] = 1.0;
    dC.upload(hc, s);
    dTmp.alloc((size_t)ld * 2);
    dTmp.zero(s);
    k::launch_modal_expand(n, B, ld, m + 2, dC.p, ldc, 2, k::MODAL_NP, dTmp.p, ld, s);
    MFH_HIP(hipMemcpyAsync(B + (int64_t)m * ld, dTmp.p, (size_t)ld * 2 * sizeof(double), hipMemcpyDeviceToDevice, s));
}

// ---- The setup the three drivers share: the loads of a call (load planes for mfh_modal_harmonic), na <= 8 columns f[a] of n doubles (null: zero). In
// the order of the steps:
//   solve    which loads are not zero off the fixed variables, and the static solves of those -- on the context's own storage, solver and
//            preconditioner, so before a caller's WideGuard. Only where a correction is wanted (then na <= 2: the basis has two reserved columns).
//   stage    the loads masked on the device, ld apart (dF: mfh_modal_harmonic takes its norms and residuals against it)
//   project  g = Phi^T f (g[j na + a]) and, after a solve, r_a into the reserved columns: the drivers then stream nb = m + na columns, else nb = m
// prepare_modal_loads makes the three in a row. The counts go to the caller's info as they grow (correction_solves).
struct ModalLoads {
    int na = 0, nb = 0, staticSolves = 0, staticIts = 0;
    bool corr = false;                  // the reserved columns hold corrections
    std::vector<double> g;
    DBuf<double> dF;
    bool nonZero[2] = {false, false};
    std::vector<double> us[2];
    DBuf<double> dC, dTmp;              // correction_columns' buffers

    void solve(mfh_ctx *c, const char *who, int na_, const double *const f[], bool wantCorrection, double rtol, int maxit, int32_t *infoSolves, int32_t *infoIts) {
        na = na_;
        if (!wantCorrection) return;
        const uint8_t *hm = c->fixedVars.empty() ? nullptr : c->hFixedMask.data();
        for (int a = 0; a < std::min(na, 2); ++a)
            for (int64_t i = 0; f[a] && i < c->modal.n && !nonZero[a]; ++i) nonZero[a] = f[a][i] != 0.0 && !(hm && hm[i]);
        correction_solves(c, who, na, f, nonZero, us, rtol, maxit, staticSolves, staticIts, infoSolves, infoIts);
    }
    void stage(mfh_ctx *c, const char *who, const double *const f[]) {
        require_basis(c, who);
        const int64_t n = c->modal.n, ld = c->modal.ld;
        dF.alloc((size_t)ld * na);
        dF.zero(c->stream);
        for (int a = 0; a < na; ++a) {
            if (f[a]) upload(dF.p + (int64_t)a * ld, f[a], n, c->stream);
            if (!c->fixedVars.empty()) k::launch_mask(n, c->dFixedMask.p, dF.p + (int64_t)a * ld, c->stream);
        }
    }
    void project(mfh_ctx *c) {
        const mfh_ctx::ModalBasis &mb = c->modal;
        g.resize((size_t)mb.nModes * na);
        gram_against(c, mb.B.p, mb.ld, mb.nModes, dF.p, mb.ld, na, 0.0, g.data());
        corr = staticSolves > 0;
        nb = corr ? mb.nModes + na : mb.nModes;
        if (corr) correction_columns(c, mb.B.p, mb.n, mb.ld, mb.nModes, na, us, nonZero, g.data(), mb.lambda.data(), dC, dTmp, c->stream);
    }
};

void prepare_modal_loads(mfh_ctx *c, const char *who, ModalLoads &L, int na, const double *const f[], bool wantCorrection, double rtol, int maxit, int32_t *infoSolves,
                         int32_t *infoIts) {
    L.solve(c, who, na, f, wantCorrection, rtol, maxit, infoSolves, infoIts);
    if (!c->fixedVars.empty()) ensure_fixed_uploaded(c);
    L.stage(c, who, f);
    L.project(c);
    if (L.corr) MFH_HIP(hipStreamSynchronize(c->stream));
}

// the probe rows of the nb columns of B, k_modal_gather_rows' layout; synchronises (probeVars is the caller's)
void gather_probe_rows(const double *B, int64_t ld, int nb, const int64_t *probeVars, int nProbe, DBuf<double> &dBp, int64_t ldp, hipStream_t s) {
    DBuf<int64_t> dProbeVars;
    dProbeVars.alloc((size_t)nProbe);
    MFH_HIP(hipMemcpyAsync(dProbeVars.p, probeVars, (size_t)nProbe * sizeof(int64_t), hipMemcpyHostToDevice, s));
    dBp.alloc((size_t)ldp * nb);
    dBp.zero(s);
    hipLaunchKernelGGL(k::k_modal_gather_rows, dim3(k::grid_for((int64_t)nProbe * nb)), dim3(256), 0, s, nProbe, nb, (const int64_t *)dProbeVars.p, B, ld, dBp.p, ldp);
    CHECK_LAUNCH();
    MFH_HIP(hipStreamSynchronize(s));
}

// ---- what the entry points refuse alike, each under its own name
void check_damping(const char *who, double aR, double bR) {
    require_for(aR >= 0.0 && bR >= 0.0 && std::isfinite(aR) && std::isfinite(bR), MFH_ERR_INVALID, who, "the Rayleigh coefficients are not negative");
}
void check_damping(const char *who, double aR, double bR, double eta) {
    check_damping(who, aR, bR);
    require_for(eta >= 0.0 && std::isfinite(eta), MFH_ERR_INVALID, who, "the loss factor is not negative");
}
void check_modal_damping(const char *who, const double *zeta, int m) {
    if (zeta)
        for (int j = 0; j < m; ++j) require_for(std::isfinite(zeta[j]) && zeta[j] >= 0.0, MFH_ERR_INVALID, who, "a damping ratio is negative or not finite");
}
void check_probes(const mfh_ctx *c, const char *who, const int64_t *probeVars, int32_t nProbe, const void *out) {
    require_for(nProbe >= 0 && (nProbe == 0 || (probeVars && out)), MFH_ERR_INVALID, who, "probes need their variables and their output");
    const int64_t nv = (int64_t)c->bs() * c->nDoF;
    for (int32_t j = 0; j < nProbe; ++j) require_for(probeVars[j] >= 0 && probeVars[j] < nv, MFH_ERR_INVALID, who, "probe variable out of range");
}
// a correction is K u = f solved: K definite (fixed variables), and the modes' share g_j / lambda_j taken out of it
void check_correctable(const mfh_ctx *c, const char *who) {
    require_for(!c->fixedVars.empty(), MFH_ERR_UNSUPPORTED, who, "the static correction needs fixed variables (K alone is singular)");
    for (double l : c->modal.lambda) require_for(l > 0.0, MFH_ERR_INVALID, who, "the static correction needs lambda_j > 0");
}

void check_sweep_params(const mfh_ctx *c, const mfh_modal_harmonic_params *p, const double *omega, const double *zeta, const double *fRe, const int64_t *probeVars,
                        int32_t nProbe, const double *probeOut) {
    require(p != nullptr, MFH_ERR_INVALID, "mfh_modal_harmonic: params is null");
    require(p->nFreq >= 0 && p->maxit > 0, MFH_ERR_INVALID, "mfh_modal_harmonic: nFreq >= 0, maxit > 0");
    check_damping("mfh_modal_harmonic", p->rayleighMass, p->rayleighStiff, p->lossFactor);
    require(p->rtol > 0.0 && p->rtol < 1.0, MFH_ERR_INVALID, "mfh_modal_harmonic: 0 < rtol < 1");
    require((p->flags & ~(MFH_MODAL_STATIC_CORRECTION | MFH_MODAL_RESIDUALS)) == 0, MFH_ERR_INVALID, "mfh_modal_harmonic: unknown flag");
    require(p->residualStride >= 0, MFH_ERR_INVALID, "mfh_modal_harmonic: residualStride >= 0");
    require(p->nFreq == 0 || omega != nullptr, MFH_ERR_INVALID, "mfh_modal_harmonic: omega is null");
    require(fRe != nullptr, MFH_ERR_INVALID, "mfh_modal_harmonic: fRe is null");
    for (int32_t k2 = 0; k2 < p->nFreq; ++k2) {
        require(std::isfinite(omega[k2]) && omega[k2] >= 0.0, MFH_ERR_INVALID, "mfh_modal_harmonic: a frequency is negative or not finite");
        require(omega[k2] > 0.0 || !c->fixedVars.empty(), MFH_ERR_INVALID, "mfh_modal_harmonic: omega = 0 needs fixed variables (K alone is singular)");
    }
    check_probes(c, "mfh_modal_harmonic", probeVars, nProbe, probeOut);
    require(!((p->flags & MFH_MODAL_RESIDUALS) && zeta), MFH_ERR_INVALID, "mfh_modal_harmonic: per-mode damping has no operator to take a residual against");
    check_modal_damping("mfh_modal_harmonic", zeta, c->modal.nModes);
}

// ---- the transient driver, shared by mfh_modal_transient and its hook. Everything on the device; the host arrays are outputs (null: not wanted).
struct MarchRun {
    int m = 0, nSteps = 0, chunk = k::MT_CHUNK;
    double dt = 0.0;
    const double *coef = nullptr, *g = nullptr, *lam = nullptr;      // device: 8 x MT_COEF_LD, m, m
    const double *amp = nullptr;                                     // device: nSteps + 1
    double *state = nullptr;                                         // device: 2 x MODAL_MAXM, in / out
    const double *Bp = nullptr; int64_t ldp = 0; int nProbe = 0; bool corr = false;
    double *probeOut = nullptr, *modalCoords = nullptr, *energies = nullptr;   // host
    int stride = 0; const double *B = nullptr; int64_t ld = 0, n = 0; int nb = 0; double *snapshots = nullptr;   // host: snapshots of n doubles
    double marchMs = 0.0, seriesMs = 0.0, expandMs = 0.0; int chunks = 0;
};

void run_march(hipStream_t s, MarchRun &R) {
    const int m = R.m, chunk = R.chunk;
    const int64_t rows = (int64_t)R.nSteps + 1;
    const int cap = (int)std::min<int64_t>(chunk, rows);
    const int stride = R.snapshots ? R.stride : 0;
    const bool series = R.nProbe > 0 || R.energies;
    DBuf<double> dSlope, dQ, dV, dCs, dProbe, dEn, dStage;
    dSlope.alloc((size_t)rows);
    hipLaunchKernelGGL(k::k_modal_slope, dim3(k::grid_for(rows)), dim3(256), 0, s, rows, R.amp, R.dt, dSlope.p);
    CHECK_LAUNCH();
    dQ.alloc((size_t)cap * m);
    if (R.energies) { dV.alloc((size_t)cap * m); dEn.alloc((size_t)cap * 3); }
    if (R.nProbe) dProbe.alloc((size_t)cap * R.nProbe);
    const int ldcs = stride ? cap / stride + 1 + k::MODAL_NP_MAX : 0;
    const int64_t snapsIn256MB = std::max<int64_t>(1, ((int64_t)1 << 25) / std::max<int64_t>(R.n, 1));
    if (stride) {
        dCs.alloc((size_t)(m + 1) * ldcs);
        dStage.alloc((size_t)std::min<int64_t>(snapsIn256MB, cap / stride + 1) * (size_t)R.n);
    }
    for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
        const int count = (int)std::min<int64_t>(chunk, rows - r0);
        int snapNext = -1, nSnap = 0;
        int64_t snap0 = 0;         // index of the chunk's first snapshot in the run
        if (stride) {
            snap0 = (r0 + stride - 1) / stride;
            const int64_t local = snap0 * stride - r0;
            if (local < count) { snapNext = (int)local; nSnap = (count - 1 - snapNext) / stride + 1; }
            dCs.zero(s);
        }
        {
            EventTimer t(s);
            hipLaunchKernelGGL(k::k_modal_march, dim3(1), dim3(256), 0, s, m, R.coef, R.g, R.amp + r0, (const double *)dSlope.p + r0, r0 == 0 ? 1 : 0, count, R.state, dQ.p,
                               dV.p, m, snapNext, std::max(stride, 1), dCs.p, ldcs);
            CHECK_LAUNCH();
            R.marchMs += t.stop();
        }
        if (series) {
            EventTimer t(s);
            k::launch_modal_series(m, count, dQ.p, dV.p, m, R.Bp, R.ldp, R.nProbe, R.corr, R.amp + r0, R.lam, R.g, dProbe.p, R.energies ? dEn.p : nullptr, s);
            R.seriesMs += t.stop();
        }
        for (int64_t c0 = 0; c0 < nSnap; c0 += snapsIn256MB) {          // the snapshots leave 256 MB at a time (one at least)
            const int np = (int)std::min<int64_t>(snapsIn256MB, nSnap - c0);
            EventTimer t(s);
            k::launch_modal_expand(R.n, R.B, R.ld, R.nb, dCs.p + c0, ldcs, np, k::MODAL_NP, dStage.p, R.n, s);
            R.expandMs += t.stop();
            MFH_HIP(hipMemcpyAsync(R.snapshots + (size_t)(snap0 + c0) * (size_t)R.n, dStage.p, (size_t)np * (size_t)R.n * sizeof(double), hipMemcpyDeviceToHost, s));
            MFH_HIP(hipStreamSynchronize(s));
        }
        if (R.nProbe) MFH_HIP(hipMemcpyAsync(R.probeOut + (size_t)r0 * R.nProbe, dProbe.p, (size_t)count * R.nProbe * sizeof(double), hipMemcpyDeviceToHost, s));
        if (R.modalCoords) MFH_HIP(hipMemcpyAsync(R.modalCoords + (size_t)r0 * m, dQ.p, (size_t)count * m * sizeof(double), hipMemcpyDeviceToHost, s));
        if (R.energies) MFH_HIP(hipMemcpyAsync(R.energies + (size_t)r0 * 3, dEn.p, (size_t)count * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        MFH_HIP(hipStreamSynchronize(s));
        ++R.chunks;
    }
}

// the coefficient table of the device, 8 x MT_COEF_LD, from rows of eight per mode
std::vector<double> coef_table(int m, const double *coef8) {
    std::vector<double> t((size_t)8 * k::MT_COEF_LD, 0.0);
    for (int j = 0; j < m; ++j)
        for (int k2 = 0; k2 < 8; ++k2) t[(size_t)k2 * k::MT_COEF_LD + j] = coef8[(size_t)j * 8 + k2];
    return t;
}

// The tables and the state of a run on the device: the coefficient table, g, lambda (null: no energies asked), the rows of the amplitude and the state
// {q, qdot} packed 2 x MODAL_MAXM (q null: rest). unpack brings the state after the run back.
struct MarchTables {
    DBuf<double> dCoef, dG, dLam, dAmp, dState;
    std::vector<double> hs;
    MarchTables(int m, const double *coef8, const double *g, const double *lam, const double *amp, int64_t rows, const double *q, const double *qdot, hipStream_t s)
        : hs((size_t)2 * k::MODAL_MAXM, 0.0) {
        dCoef.upload(coef_table(m, coef8), s);
        dG.upload(g, (size_t)m, s);
        if (lam) dLam.upload(lam, (size_t)m, s);
        dAmp.upload(amp, (size_t)rows, s);
        if (q) { std::copy(q, q + m, hs.begin()); std::copy(qdot, qdot + m, hs.begin() + k::MODAL_MAXM); }
        dState.upload(hs, s);
    }
    void point(MarchRun &R) const { R.coef = dCoef.p; R.g = dG.p; R.lam = dLam.p; R.amp = dAmp.p; R.state = dState.p; }
    void unpack(int m, double *q, double *qdot, hipStream_t s) {
        dState.download(hs.data(), hs.size(), s);
        std::copy(hs.begin(), hs.begin() + m, q);
        std::copy(hs.begin() + k::MODAL_MAXM, hs.begin() + k::MODAL_MAXM + m, qdot);
    }
};

using BasisFill = std::function<void(double *, int64_t, hipStream_t)>;
void install_basis(mfh_ctx *c, const char *who, int32_t nModes, const double *lambda, double density, mfh_modal_basis_info *info, const BasisFill &fill);

bool chunk_ok(int32_t chunkSteps) { return chunkSteps == 0 || (chunkSteps > 0 && chunkSteps % 32 == 0); }

}   // namespace

extern "C" {

mfh_status mfh_modal_transient(mfh_ctx *c, const mfh_modal_transient_params *prm, const double *modalDamping, double *q, double *qdot, const double *f,
                               const double *amplitude, const int64_t *probeVars, int32_t nProbe, double *probeOut, double *snapshots, double *modalCoords,
                               double *energies, mfh_modal_transient_info *info) {
    if (info) { *info = mfh_modal_transient_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_modal_transient: null context");
    require(prm != nullptr, MFH_ERR_INVALID, "mfh_modal_transient: params is null");
    const mfh_modal_transient_params P = *prm;
    require(P.dt > 0.0 && std::isfinite(P.dt), MFH_ERR_INVALID, "mfh_modal_transient: dt > 0");
    require(P.nSteps >= 0 && P.snapshotStride >= 0 && P.maxit >= 0 && nProbe >= 0, MFH_ERR_INVALID, "mfh_modal_transient: a count or the stride is negative");
    check_damping("mfh_modal_transient", P.rayleighMass, P.rayleighStiff);
    require((P.flags & ~(MFH_MODAL_TR_STATIC_CORRECTION | MFH_MODAL_TR_ENERGIES)) == 0, MFH_ERR_INVALID, "mfh_modal_transient: unknown flag");
    require(chunk_ok(P.chunkSteps), MFH_ERR_INVALID, "mfh_modal_transient: chunkSteps is 0 or a positive multiple of 32");
    require((q == nullptr) == (qdot == nullptr), MFH_ERR_INVALID, "mfh_modal_transient: q and qdot come together");
    const bool correct = (P.flags & MFH_MODAL_TR_STATIC_CORRECTION) != 0, wantEn = (P.flags & MFH_MODAL_TR_ENERGIES) != 0;
    require(wantEn == (energies != nullptr), MFH_ERR_INVALID, "mfh_modal_transient: the energies and MFH_MODAL_TR_ENERGIES come together");
    require(!correct || (P.rtol > 0.0 && P.rtol < 1.0 && P.maxit > 0), MFH_ERR_INVALID, "mfh_modal_transient: the static solve needs 0 < rtol < 1, maxit > 0");
    require(f != nullptr, MFH_ERR_INVALID, "mfh_modal_transient: f is null");
    require(!snapshots || P.snapshotStride > 0, MFH_ERR_INVALID, "mfh_modal_transient: snapshots need snapshotStride > 0");
    check_probes(c, "mfh_modal_transient", probeVars, nProbe, probeOut);
    if (amplitude) require(all_finite(amplitude, (int64_t)P.nSteps + 1), MFH_ERR_INVALID, "mfh_modal_transient: an amplitude is not finite");
    check_modal_damping("mfh_modal_transient", modalDamping, c->modal.nModes);       // (a basis of another length is caught below; the entries a basis could have are at most MODAL_MAXM)
    prepare_pencil(c, "mfh_modal_transient");
    require_basis(c, "mfh_modal_transient");
    const int m = c->modal.nModes;
    const int64_t n = c->modal.n, ld = c->modal.ld;
    const std::vector<double> lam = c->modal.lambda;
    if (correct) check_correctable(c, "mfh_modal_transient");
    require(all_finite(f, n), MFH_ERR_INVALID, "mfh_modal_transient: the load has an entry that is not finite");
    if (q) require(all_finite(q, m) && all_finite(qdot, m), MFH_ERR_INVALID, "mfh_modal_transient: the start state has an entry that is not finite");
    // the eight coefficients per mode, on the host
    std::vector<double> coef8((size_t)m * 8);
    for (int j = 0; j < m; ++j) {
        const double l = lam[(size_t)j], cj = P.rayleighMass + P.rayleighStiff * l + (modalDamping ? 2.0 * modalDamping[j] * std::sqrt(l) : 0.0);
        require(std::isfinite(cj) && mfh_modal_transient_coeffs(l, cj, P.dt, coef8.data() + (size_t)j * 8) == MFH_OK, MFH_ERR_INVALID,
                "mfh_modal_transient: the damping of a mode is not finite");
    }
    hipStream_t s = c->stream;
    c->modalNote.clear();
    EventTimer tsetup(s);

    // ---- the load: g = Phi^T f and, with a correction, r_s = u_s - sum_j phi_j g_j / lambda_j in the first reserved column (the second one zero:
    // the m + 1 columns streamed from here on leave it out)
    ModalLoads L;
    prepare_modal_loads(c, "mfh_modal_transient", L, 1, &f, correct, P.rtol, P.maxit, info ? &info->staticSolves : nullptr, info ? &info->staticIterations : nullptr);
    if (L.corr) modal_note(c, "static correction: 1 solve of K u = f, " + std::to_string(L.staticIts) + " iterations");
    const double *const B = c->modal.B.p;
    const int nb = L.nb;

    // ---- the probe rows of B, gathered once
    DBuf<double> dBp;
    const int64_t ldp = ((int64_t)nProbe + 31) / 32 * 32;
    if (nProbe) gather_probe_rows(B, ld, nb, probeVars, nProbe, dBp, ldp, s);

    // ---- tables and state
    std::vector<double> ones;
    if (!amplitude) ones.assign((size_t)P.nSteps + 1, 1.0);
    MarchTables T(m, coef8.data(), L.g.data(), lam.data(), amplitude ? amplitude : ones.data(), (int64_t)P.nSteps + 1, q, qdot, s);
    const double setupMs = tsetup.stop();

    MarchRun R;
    R.m = m; R.nSteps = P.nSteps; R.chunk = P.chunkSteps ? P.chunkSteps : k::MT_CHUNK; R.dt = P.dt;
    T.point(R);
    R.Bp = dBp.p; R.ldp = ldp; R.nProbe = nProbe; R.corr = L.corr;
    R.probeOut = probeOut; R.modalCoords = modalCoords; R.energies = energies;
    R.stride = P.snapshotStride; R.B = B; R.ld = ld; R.n = n; R.nb = nb; R.snapshots = snapshots;
    run_march(s, R);
    if (q) T.unpack(m, q, qdot, s);
    if (info) {
        info->stepsDone = P.nSteps; info->staticSolves = L.staticSolves; info->staticIterations = L.staticIts;
        info->chunkSteps = R.chunk; info->chunks = R.chunks;
        info->setupMs = setupMs; info->marchMs = R.marchMs; info->seriesMs = R.seriesMs; info->expandMs = R.expandMs;
        info->note = c->modalNote.c_str();
    }
    MFH_CATCH(c)
}

mfh_status mfh_debug_modal_march(mfh_ctx *c, int32_t nModes, const double *coef8, const double *g, const double *lambda, double dt, int32_t nSteps,
                                 const double *amplitude, int32_t chunkSteps, double *q, double *qdot, const double *Bp, int32_t nProbe, int32_t corr,
                                 double *modalCoords, double *probeOut, double *energies) {
    MFH_TRY(c)
    require(c && coef8 && g && amplitude && q && qdot && nModes >= 1 && nModes <= k::MODAL_MAXM && nSteps >= 0 && dt > 0.0 && chunk_ok(chunkSteps) && nProbe >= 0 &&
                (nProbe == 0 || (Bp && probeOut)) && (!energies || lambda) && (corr == 0 || corr == 1),
            MFH_ERR_INVALID, "mfh_debug_modal_march: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int m = nModes, nb = m + corr;
    const int64_t ldp = ((int64_t)nProbe + 31) / 32 * 32;
    MarchTables T(m, coef8, g, lambda, amplitude, (int64_t)nSteps + 1, q, qdot, s);
    DBuf<double> dBp;
    if (nProbe) {          // Bp: nb rows of nProbe (row j = column j of the basis at the probe variables)
        dBp.alloc((size_t)ldp * nb);
        dBp.zero(s);
        upload_columns(dBp.p, ldp, Bp, nProbe, nb, s);
        MFH_HIP(hipStreamSynchronize(s));
    }
    MarchRun R;
    R.m = m; R.nSteps = nSteps; R.chunk = chunkSteps ? chunkSteps : k::MT_CHUNK; R.dt = dt;
    T.point(R);
    R.Bp = dBp.p; R.ldp = ldp; R.nProbe = nProbe; R.corr = corr != 0;
    R.probeOut = probeOut; R.modalCoords = modalCoords; R.energies = energies;
    run_march(s, R);
    T.unpack(m, q, qdot, s);
    MFH_CATCH(c)
}

// ms per repetition of (a) k_modal_series and (b) the k_modal_expand route (the gathered rows as the kernel's rows, 32 steps per pass) for nProbe probes of
// nSteps rows on nb hashed columns, the two taking turns
mfh_status mfh_time_modal_series(mfh_ctx *c, int32_t nModes, int32_t nProbe, int32_t nSteps, int32_t reps, double *seriesMs, double *expandMs) {
    MFH_TRY(c)
    require(c && seriesMs && expandMs && nModes >= 1 && nModes <= k::MODAL_MAXM && nProbe >= 1 && nProbe <= 4096 && nSteps >= 1 && reps >= 1, MFH_ERR_INVALID,
            "mfh_time_modal_series: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int m = nModes;
    const int64_t ldp = ((int64_t)nProbe + 31) / 32 * 32;
    const int ldc = nSteps + k::MODAL_NP_MAX;
    DBuf<double> dQ, dCt, dBp, dAmp, dOut;
    dQ.alloc((size_t)nSteps * m); dCt.alloc((size_t)m * ldc); dBp.alloc((size_t)ldp * m); dAmp.alloc((size_t)nSteps); dOut.alloc((size_t)nSteps * nProbe);
    k::launch_fill_hash((int64_t)dQ.n, dQ.p, s);
    k::launch_fill_hash((int64_t)dCt.n, dCt.p, s);
    k::launch_fill_hash((int64_t)dBp.n, dBp.p, s);
    k::launch_fill_hash((int64_t)dAmp.n, dAmp.p, s);
    auto a = [&] { k::launch_modal_series(m, nSteps, dQ.p, nullptr, m, dBp.p, ldp, nProbe, false, dAmp.p, nullptr, nullptr, dOut.p, nullptr, s); };
    auto b = [&] { k::launch_modal_expand(nProbe, dBp.p, ldp, m, dCt.p, ldc, nSteps, k::MODAL_NP, dOut.p, nProbe, s); };
    a(); b();          // warm-up
    MFH_HIP(hipStreamSynchronize(s));
    for (int r = 0; r < reps; ++r) {
        { EventTimer t(s); a(); seriesMs[r] = t.stop(); }
        { EventTimer t(s); b(); expandMs[r] = t.stop(); }
    }
    MFH_CATCH(c)
}

mfh_status mfh_modal_set_basis(mfh_ctx *c, int32_t nModes, const double *lambda, const double *X, double density, mfh_modal_basis_info *info) {
    if (info) *info = mfh_modal_basis_info{};
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_modal_set_basis: null context");
    require(nModes >= 0 && nModes <= k::MODAL_MAXM, MFH_ERR_INVALID, "mfh_modal_set_basis: 0 <= nModes <= 256");
    if (nModes == 0) { modal_drop(c); return MFH_OK; }
    require(lambda && X, MFH_ERR_INVALID, "mfh_modal_set_basis: lambda and X are needed");
    require(density > 0.0 && std::isfinite(density), MFH_ERR_INVALID, "mfh_modal_set_basis: density > 0");
    for (int j = 0; j < nModes; ++j) require(std::isfinite(lambda[j]) && lambda[j] >= 0.0, MFH_ERR_INVALID, "mfh_modal_set_basis: an eigenvalue is negative or not finite");
    prepare_pencil(c, "mfh_modal_set_basis");
    const int64_t n = (int64_t)c->bs() * c->nDoF;
    require(all_finite(X, (int64_t)nModes * n), MFH_ERR_INVALID, "mfh_modal_set_basis: a mode has an entry that is not finite");
    install_basis(c, "mfh_modal_set_basis", nModes, lambda, density, info, [&](double *B, int64_t ld, hipStream_t s) { upload_columns(B, ld, X, n, nModes, s); });
    MFH_CATCH(c)
}

mfh_status mfh_modal_set_basis_from_modes(mfh_ctx *c, int32_t nModes, double density, mfh_modal_basis_info *info) {
    if (info) *info = mfh_modal_basis_info{};
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_modal_set_basis_from_modes: null context");
    require(nModes >= 1 && nModes <= k::MODAL_MAXM, MFH_ERR_INVALID, "mfh_modal_set_basis_from_modes: 1 <= nModes <= 256");
    require(density > 0.0 && std::isfinite(density), MFH_ERR_INVALID, "mfh_modal_set_basis_from_modes: density > 0");
    prepare_pencil(c, "mfh_modal_set_basis_from_modes");
    const mfh_ctx::ModesKeep &kp = c->modesKeep;
    const int64_t n = (int64_t)c->bs() * c->nDoF;
    require(kp.Q.p != nullptr && !kp.src.empty(), MFH_ERR_STATE, "mfh_modal_set_basis_from_modes: no modes on the device (the context's last mfh_modes_many did not converge, or none was made)");
    require(c->geoValid && kp.geoGen == c->geoGen && kp.densityGen == c->densityGen && kp.n == n && sorted_fixed(c) == kp.fixedSet, MFH_ERR_STATE,
            "mfh_modal_set_basis_from_modes: the modes on the device are stale (vertex positions, material, density field, DoF map or the set of fixed variables changed since mfh_modes_many)");
    require(nModes <= (int)kp.src.size(), MFH_ERR_INVALID, "mfh_modal_set_basis_from_modes: more modes than mfh_modes_many found");
    const std::vector<double> lam(kp.lambda.begin(), kp.lambda.begin() + nModes);
    for (double l : lam) require(std::isfinite(l) && l >= 0.0, MFH_ERR_INVALID, "mfh_modal_set_basis_from_modes: an eigenvalue is negative or not finite");
    install_basis(c, "mfh_modal_set_basis_from_modes", nModes, lam.data(), density, info, [&](double *B, int64_t ld, hipStream_t s) {
        require(ld == kp.ld, MFH_ERR_STATE, "mfh_modal_set_basis_from_modes: the column stride changed");
        for (int j = 0; j < nModes; ++j)
            hipLaunchKernelGGL(k::k_modal_adopt, dim3(k::grid_for(n)), dim3(256), 0, s, n, (const double *)kp.Q.p + (int64_t)kp.src[(size_t)j] * kp.ld, kp.sign[(size_t)j],
                               B + (int64_t)j * ld);
        CHECK_LAUNCH();
    });
    MFH_CATCH(c)
}

}   // extern "C"

namespace {

// The common part of mfh_modal_set_basis and mfh_modal_set_basis_from_modes: fill(B, ld, stream) writes the nModes columns; then the fixed rows are
// zeroed, orthoDefect formed and the state recorded.
void install_basis(mfh_ctx *c, const char *who, int32_t nModes, const double *lambda, double density, mfh_modal_basis_info *info, const BasisFill &fill) {
    const int64_t n = (int64_t)c->bs() * c->nDoF, ld = (n + 31) / 32 * 32;
    hipStream_t s = c->stream;
    modal_drop(c);
    WideGuard guard(c);
    EventTimer tsetup(s);
    prepare_pencil_state(c, who, false);
    mfh_ctx::ModalBasis &mb = c->modal;
    mb.B.alloc((size_t)ld * (size_t)(nModes + 2));
    mb.B.zero(s);
    fill(mb.B.p, ld, s);
    if (!c->fixedVars.empty())
        for (int j = 0; j < nModes; ++j) k::launch_mask(n, c->dFixedMask.p, mb.B.p + (int64_t)j * ld, s);
    std::vector<double> G((size_t)nModes * nModes);
    gram_against(c, mb.B.p, ld, nModes, mb.B.p, ld, nModes, density, G.data());
    double defect = 0.0;
    for (int i = 0; i < nModes; ++i)
        for (int j = 0; j < nModes; ++j) {
            const double e = std::fabs(G[(size_t)i * nModes + j] - (i == j ? 1.0 : 0.0));
            defect = std::isfinite(e) ? std::max(defect, e) : e;
        }
    mb.nModes = nModes; mb.n = n; mb.ld = ld; mb.density = density;
    mb.lambda.assign(lambda, lambda + nModes);
    mb.geoGen = c->geoGen; mb.densityGen = c->densityGen;
    mb.fixedSet = sorted_fixed(c);
    if (info) {
        info->nModes = nModes; info->ld = ld; info->orthoDefect = defect;
        info->deviceBytes = (double)mb.B.n * sizeof(double);
        info->setupMs = tsetup.stop();
    }
}

}   // namespace

extern "C" {

mfh_status mfh_modal_coordinates(mfh_ctx *c, const double *u, int32_t nVec, double *q) {
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_modal_coordinates: null context");
    require(nVec >= 0, MFH_ERR_INVALID, "mfh_modal_coordinates: nVec >= 0");
    prepare_pencil(c, "mfh_modal_coordinates");
    require_basis(c, "mfh_modal_coordinates");
    require(nVec == 0 || (u && q), MFH_ERR_INVALID, "mfh_modal_coordinates: u and q are needed");
    if (nVec == 0) return MFH_OK;
    hipStream_t s = c->stream;
    WideGuard guard(c);
    prepare_pencil_state(c, "mfh_modal_coordinates", false);
    require_basis(c, "mfh_modal_coordinates");
    const mfh_ctx::ModalBasis &mb = c->modal;
    const int m = mb.nModes;
    DBuf<double> du;
    du.alloc((size_t)mb.ld * k::MG_TV);
    du.zero(s);
    std::vector<double> G((size_t)m * k::MG_TV);
    for (int v0 = 0; v0 < nVec; v0 += k::MG_TV) {
        const int nv = std::min(k::MG_TV, nVec - v0);
        upload_columns(du.p, mb.ld, u + (size_t)v0 * (size_t)mb.n, mb.n, nv, s);
        gram_against(c, mb.B.p, mb.ld, m, du.p, mb.ld, nv, mb.density, G.data());
        for (int j = 0; j < nv; ++j)
            for (int i = 0; i < m; ++i) q[(size_t)(v0 + j) * m + i] = G[(size_t)i * nv + j];
    }
    MFH_CATCH(c)
}

mfh_status mfh_modal_harmonic(mfh_ctx *c, const mfh_modal_harmonic_params *prm, const double *omega, const double *modalDamping, const double *fRe, const double *fIm,
                              const int64_t *probeVars, int32_t nProbe, double *probeOut, double *fields, double *modalCoords, double *trueResiduals,
                              mfh_modal_harmonic_info *info) {
    if (info) { *info = mfh_modal_harmonic_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_modal_harmonic: null context");
    check_sweep_params(c, prm, omega, modalDamping, fRe, probeVars, nProbe, probeOut);
    const mfh_modal_harmonic_params P = *prm;
    prepare_pencil(c, "mfh_modal_harmonic");
    require_basis(c, "mfh_modal_harmonic");
    const bool correct = (P.flags & MFH_MODAL_STATIC_CORRECTION) != 0, wantRes = (P.flags & MFH_MODAL_RESIDUALS) != 0;
    const bool masked = !c->fixedVars.empty();
    const int m = c->modal.nModes, nFreq = P.nFreq;
    const int64_t n = c->modal.n, ld = c->modal.ld;
    const std::vector<double> lam = c->modal.lambda;
    const double density = c->modal.density;
    if (correct) check_correctable(c, "mfh_modal_harmonic");
    // the denominators: nModes x nFreq complex scalars, refused before any device work where one is zero
    std::vector<Cplx> dinv((size_t)std::max(nFreq, 1) * m);
    for (int k2 = 0; k2 < nFreq; ++k2) {
        const double w = omega[k2];
        for (int j = 0; j < m; ++j) {
            const double l = lam[(size_t)j];
            require(w > 0.0 || l > 0.0, MFH_ERR_INVALID, "mfh_modal_harmonic: omega = 0 with a zero eigenvalue in the basis");
            const Cplx d = modal_d(l, w, P.rayleighMass, P.rayleighStiff, P.lossFactor, modalDamping ? modalDamping[j] : 0.0);
            require(d.re != 0.0 || d.im != 0.0, MFH_ERR_INVALID, "mfh_modal_harmonic: an undamped frequency sits on an eigenfrequency of the basis (d_j = 0)");
            dinv[(size_t)k2 * m + j] = crecip(d);
        }
    }
    hipStream_t s = c->stream;
    c->modalNote.clear();
    EventTimer tsetup(s);

    // ---- the static solves, as mfh_solve makes them (outside the WideGuard: the context's own storage, solver and preconditioner)
    ModalLoads L;
    const double *const fPlane[2] = {fRe, fIm};
    L.solve(c, "mfh_modal_harmonic", 2, fPlane, correct, P.rtol, P.maxit, info ? &info->staticSolves : nullptr, info ? &info->staticIterations : nullptr);

    std::optional<WideGuard> guard;        // (the operator product of the residuals alone needs both triangles: a sweep without them leaves the storage alone)
    if (wantRes) {
        guard.emplace(c);
        if (guard->widened) modal_note(c, "the pattern held the upper triangle only: symbolic phase re-run with both triangles (what option matrix_storage 0 does) for this call");
        prepare_pencil_state(c, "mfh_modal_harmonic", false);
        if (c->harmTwoPass) modal_note(c, "mass product of the residuals: two real passes and a combine kernel (option harmonic_two_pass)");
    } else if (masked) ensure_fixed_uploaded(c);

    // ---- the load, its modal coordinates g = Phi^T f^ and its norm
    L.stage(c, "mfh_modal_harmonic", fPlane);
    const double *const B = c->modal.B.p;
    const DBuf<double> &dF = L.dF;
    DBuf<double> dPart, dScal;
    dPart.alloc((size_t)k::DYN_GRID_CAP * k::DYN_NV);
    dScal.alloc((size_t)std::max(nFreq, 1) + 1);
    dScal.zero(s);
    const int vgrid = k::dyn_grid(n, std::max(1, std::min(c->dynGridCap, k::DYN_GRID_CAP)));
    hipLaunchKernelGGL(k::k_modal_resnorm, dim3(vgrid), dim3(256), 0, s, n, (const double *)dF.p, (const double *)nullptr, ld, dPart.p);
    CHECK_LAUNCH();
    k::launch_sum(vgrid, dPart.p, k::dyn_open(), s, dScal.p + nFreq);
    double hbb = 0.0;
    MFH_HIP(hipMemcpyAsync(&hbb, dScal.p + nFreq, sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    require(std::isfinite(hbb), MFH_ERR_INVALID, "mfh_modal_harmonic: the load has an entry that is not finite");
    // ---- g[2 j + plane], and the static correction r_s = u_s - sum_j phi_j g_j / lambda_j in the two reserved columns, streamed (nb = m + 2) only
    // where they hold something
    L.project(c);
    const std::vector<double> &g = L.g;
    const int nb = L.nb;
    if (L.corr) modal_note(c, "static correction: " + std::to_string(L.staticSolves) + " solve(s) of K u = f, " + std::to_string(L.staticIts) + " iterations");

    // ---- probes: the rows of B at the probe variables, gathered once
    DBuf<double> dBp, dProbe, dC;
    const int64_t ldp = ((int64_t)nProbe + 31) / 32 * 32;
    if (nProbe && nFreq) {
        gather_probe_rows(B, ld, nb, probeVars, nProbe, dBp, ldp, s);
        dProbe.alloc((size_t)nFreq * 2 * (size_t)nProbe);
    }

    // ---- the sweep, in groups of frequencies: staging rows {re plane, im plane} of n doubles each -- 256 MB as in mfh_harmonic, but the planes of
    // one full pass of the kernel at least (the basis is streamed once per pass: a group of one frequency would read it for two planes)
    const int64_t rowLen = 2 * n;
    const bool staging = fields != nullptr || wantRes;
    const int64_t rowsIn256MB = std::max<int64_t>(1, ((int64_t)1 << 25) / std::max<int64_t>(rowLen, 1));
    int groupCap = (int)std::min<int64_t>(MODAL_GROUP_MAX, staging ? std::max<int64_t>(k::MODAL_NP / 2, rowsIn256MB) : MODAL_GROUP_MAX);
    DBuf<double> dStage, dX, dY, dT;
    if (staging && nFreq) {
        // where the device has no room for the rows of a full pass (5.7 GB at 22.3 M unknowns), the group shrinks to what 256 MB hold: more
        // passes over the basis, the same bits
        try { dStage.alloc((size_t)std::min(groupCap, nFreq) * (size_t)rowLen); }
        catch (const Error &) {
            if (groupCap <= rowsIn256MB) throw;
            groupCap = (int)rowsIn256MB;
            dStage.alloc((size_t)std::min(groupCap, nFreq) * (size_t)rowLen);
            modal_note(c, "no device memory for the staging rows of a full pass: groups of " + std::to_string(groupCap) + " frequency(ies)");
        }
    }
    const int ldc = 2 * groupCap + k::MODAL_NP_MAX;
    if (wantRes) { dX.alloc((size_t)ld * 2); dY.alloc((size_t)ld * 2); dT.alloc((size_t)ld * 2); dX.zero(s); dY.zero(s); dT.zero(s); }
    std::vector<double> hc((size_t)nb * ldc);
    const int stride = std::max(1, (int)P.residualStride);
    const double setupMs = tsetup.stop();

    EventTimer tsolve(s);
    int groups = 0;
    for (int k0 = 0; k0 < nFreq; k0 += groupCap) {
        const int gN = std::min(groupCap, nFreq - k0);
        std::fill(hc.begin(), hc.end(), 0.0);
        for (int kk = 0; kk < gN; ++kk) {
            const int k2 = k0 + kk;
            const double w = omega[k2];
            for (int j = 0; j < m; ++j) {
                const Cplx di = dinv[(size_t)k2 * m + j], gj{g[(size_t)2 * j], g[(size_t)2 * j + 1]};
                const Cplx q{gj.re * di.re - gj.im * di.im, gj.re * di.im + gj.im * di.re};
                hc[(size_t)j * ldc + 2 * kk] = q.re;
                hc[(size_t)j * ldc + 2 * kk + 1] = q.im;
                if (modalCoords) { modalCoords[((size_t)k2 * m + j) * 2] = q.re; modalCoords[((size_t)k2 * m + j) * 2 + 1] = q.im; }
            }
            if (L.corr) {       // the real 2 x 2 form of 1 / zK on the two correction rows
                const Cplx iz = inv_zK(w, P.rayleighStiff, P.lossFactor);
                hc[(size_t)m * ldc + 2 * kk] = iz.re;       hc[(size_t)(m + 1) * ldc + 2 * kk] = -iz.im;
                hc[(size_t)m * ldc + 2 * kk + 1] = iz.im;   hc[(size_t)(m + 1) * ldc + 2 * kk + 1] = iz.re;
            }
        }
        dC.upload(hc, s);
        if (staging) k::launch_modal_expand(n, B, ld, nb, dC.p, ldc, 2 * gN, k::MODAL_NP, dStage.p, n, s);
        if (nProbe) k::launch_modal_expand(nProbe, dBp.p, ldp, nb, dC.p, ldc, 2 * gN, k::MODAL_NP, dProbe.p + (size_t)k0 * 2 * (size_t)nProbe, nProbe, s);
        if (wantRes)
            for (int kk = 0; kk < gN; ++kk) {
                const int k2 = k0 + kk;
                if (k2 % stride != 0) continue;
                const double w = omega[k2];
                const double zK[2] = {1.0, P.lossFactor + w * P.rayleighStiff}, zM[2] = {-density * w * w, density * w * P.rayleighMass};
                MFH_HIP(hipMemcpyAsync(dX.p, dStage.p + (size_t)kk * (size_t)rowLen, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
                MFH_HIP(hipMemcpyAsync(dX.p + ld, dStage.p + (size_t)kk * (size_t)rowLen + (size_t)n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
                harmonic_product(c, masked, zK, zM, dX.p, dY.p, ld, dT.p);
                hipLaunchKernelGGL(k::k_modal_resnorm, dim3(vgrid), dim3(256), 0, s, n, (const double *)dF.p, (const double *)dY.p, ld, dPart.p);
                CHECK_LAUNCH();
                k::launch_sum(vgrid, dPart.p, k::dyn_open(), s, dScal.p + k2);
            }
        if (fields)       // the rows leave 256 MB at a time (one row at least)
            for (int64_t r0 = 0; r0 < gN; r0 += rowsIn256MB) {
                const int64_t nr = std::min<int64_t>(rowsIn256MB, gN - r0);
                MFH_HIP(hipMemcpyAsync(fields + (size_t)(k0 + r0) * (size_t)rowLen, dStage.p + (size_t)r0 * (size_t)rowLen, (size_t)nr * (size_t)rowLen * sizeof(double),
                                       hipMemcpyDeviceToHost, s));
            }
        MFH_HIP(hipStreamSynchronize(s));
        ++groups;
    }
    if (nProbe && nFreq) {          // device layout [frequency][plane][probe] -> probeOut [frequency][probe][{re, im}]
        std::vector<double> hp((size_t)nFreq * 2 * (size_t)nProbe);
        dProbe.download(hp.data(), hp.size(), s);
        for (int k2 = 0; k2 < nFreq; ++k2)
            for (int j = 0; j < nProbe; ++j)
                for (int pl = 0; pl < 2; ++pl) probeOut[((size_t)k2 * nProbe + j) * 2 + pl] = hp[((size_t)k2 * 2 + pl) * nProbe + j];
    }
    double worst = 0.0;
    if (trueResiduals) std::fill(trueResiduals, trueResiduals + nFreq, -1.0);
    if (wantRes && nFreq) {
        std::vector<double> hr((size_t)nFreq);
        dScal.download(hr.data(), (size_t)nFreq, s);
        for (int k2 = 0; k2 < nFreq; k2 += stride) {
            const double t = hbb > 0.0 ? std::sqrt(hr[(size_t)k2] / hbb) : 0.0;
            if (trueResiduals) trueResiduals[k2] = t;
            worst = std::isfinite(t) ? std::max(worst, t) : t;
        }
    }
    const double solveMs = tsolve.stop();
    if (info) {
        info->staticSolves = L.staticSolves; info->staticIterations = L.staticIts;
        info->groups = groups; info->planesPerPass = k::MODAL_NP;
        info->worstTrueResidual = worst; info->setupMs = setupMs; info->solveMs = solveMs;
        info->note = c->modalNote.c_str();
    }
    MFH_CATCH(c)
}

// ---------------------------------------------------------------- quadratic forms, random vibration (docs/design/04_23_modal_random.md)
}   // extern "C"

namespace {

struct Factor {
    std::vector<double> F;
    std::vector<int32_t> piv;
    int32_t rank = 0;
    double truncation = 0.0;
};
Factor factor_or_throw(int nb, const double *C, double tol, const char *who) {
    Factor f;
    f.F.assign((size_t)nb * nb, 0.0);
    f.piv.assign((size_t)nb, 0);
    const mfh_status st = mfh_psd_factor(nb, C, tol, f.F.data(), &f.rank, f.piv.data(), &f.truncation);
    if (st != MFH_OK) throw Error(st, std::string(who) + ": a matrix is not positive semi-definite (a remaining diagonal below -tol) or has an entry that is not finite");
    return f;
}

}   // namespace

extern "C" {

mfh_status mfh_modal_quadratic(mfh_ctx *c, int32_t nMat, const double *C, double tol, const int64_t *probeVars, int32_t nProbe, double *probeOut, double *fields,
                               mfh_modal_quadratic_info *info) {
    if (info) *info = mfh_modal_quadratic_info{};
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_modal_quadratic: null context");
    require(nMat >= 1 && nMat <= 4 && C != nullptr, MFH_ERR_INVALID, "mfh_modal_quadratic: 1 <= nMat <= 4 matrices");
    require(!std::isnan(tol), MFH_ERR_INVALID, "mfh_modal_quadratic: tol is not a number");
    check_probes(c, "mfh_modal_quadratic", probeVars, nProbe, probeOut);
    prepare_pencil(c, "mfh_modal_quadratic");
    require_basis(c, "mfh_modal_quadratic");
    const int m = c->modal.nModes;
    const int64_t n = c->modal.n, ld = c->modal.ld;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Factor> fac;
    for (int a = 0; a < nMat; ++a) fac.push_back(factor_or_throw(m, C + (size_t)a * m * m, tol, "mfh_modal_quadratic"));
    const double factorMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    hipStream_t s = c->stream;
    const double *B = c->modal.B.p;
    DBuf<double> dBp, dOut, dPout;
    const int64_t ldp = ((int64_t)nProbe + 31) / 32 * 32;
    if (nProbe) { gather_probe_rows(B, ld, m, probeVars, nProbe, dBp, ldp, s); dPout.alloc((size_t)nProbe); }
    if (fields) dOut.alloc((size_t)ld);
    EventTimer tsolve(s);
    for (int a = 0; a < nMat; ++a) {
        k::SumsqPlan plan;
        plan.build(m, fac[(size_t)a].F.data(), m, fac[(size_t)a].rank, fac[(size_t)a].piv.data(), k::MODAL_NP, s);
        if (fields) {
            plan.run(n, B, ld, true, dOut.p, s);
            MFH_HIP(hipMemcpyAsync(fields + (size_t)a * (size_t)n, dOut.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        if (nProbe) {
            plan.run(nProbe, dBp.p, ldp, true, dPout.p, s);
            MFH_HIP(hipMemcpyAsync(probeOut + (size_t)a * nProbe, dPout.p, (size_t)nProbe * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        MFH_HIP(hipStreamSynchronize(s));
        if (info) { info->ranks[a] = fac[(size_t)a].rank; info->passes[a] = plan.passes; info->truncation[a] = fac[(size_t)a].truncation; }
    }
    const double solveMs = tsolve.stop();
    if (info) { info->factorMs = factorMs; info->solveMs = solveMs; }
    MFH_CATCH(c)
}

mfh_status mfh_modal_random(mfh_ctx *c, const mfh_modal_random_params *prm, const double *omega, const double *weights, const double *modalDamping, const double *f,
                            const double *S, const int64_t *probeVars, int32_t nProbe, double *probeRms, double *probePsd, double *rmsFields, double *cov,
                            mfh_modal_random_info *info) {
    if (info) { *info = mfh_modal_random_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_modal_random: null context");
    require(prm != nullptr, MFH_ERR_INVALID, "mfh_modal_random: params is null");
    const mfh_modal_random_params P = *prm;
    require(P.nFreq >= 1 && P.maxit > 0, MFH_ERR_INVALID, "mfh_modal_random: nFreq >= 1, maxit > 0");
    require(P.nLoad >= 1 && P.nLoad <= 8, MFH_ERR_INVALID, "mfh_modal_random: 1 <= nLoad <= 8");
    check_damping("mfh_modal_random", P.rayleighMass, P.rayleighStiff, P.lossFactor);
    require(P.rtol > 0.0 && P.rtol < 1.0, MFH_ERR_INVALID, "mfh_modal_random: 0 < rtol < 1");
    require(!std::isnan(P.tol), MFH_ERR_INVALID, "mfh_modal_random: tol is not a number");
    require((P.flags & ~(MFH_MODAL_RV_STATIC_CORRECTION | MFH_MODAL_RV_VELOCITY | MFH_MODAL_RV_ACCELERATION)) == 0, MFH_ERR_INVALID, "mfh_modal_random: unknown flag");
    require(omega && f && S, MFH_ERR_INVALID, "mfh_modal_random: omega, f and S are needed");
    const bool correct = (P.flags & MFH_MODAL_RV_STATIC_CORRECTION) != 0, wantV = (P.flags & MFH_MODAL_RV_VELOCITY) != 0, wantA = (P.flags & MFH_MODAL_RV_ACCELERATION) != 0;
    require(!(correct && P.nLoad > 2), MFH_ERR_UNSUPPORTED, "mfh_modal_random: the static correction has two reserved columns: at most two loads with it");
    const int nFreq = P.nFreq, nl = P.nLoad;
    for (int32_t k2 = 0; k2 < nFreq; ++k2) {
        require(std::isfinite(omega[k2]) && omega[k2] >= 0.0, MFH_ERR_INVALID, "mfh_modal_random: a frequency is negative or not finite");
        require(k2 == 0 || omega[k2] > omega[k2 - 1], MFH_ERR_INVALID, "mfh_modal_random: the frequencies are not ascending");
        require(omega[k2] > 0.0 || !c->fixedVars.empty(), MFH_ERR_INVALID, "mfh_modal_random: omega = 0 needs fixed variables (K alone is singular)");
    }
    check_probes(c, "mfh_modal_random", probeVars, nProbe, probeRms);
    require(nProbe > 0 || !probePsd, MFH_ERR_INVALID, "mfh_modal_random: the response spectra belong to probes");
    check_modal_damping("mfh_modal_random", modalDamping, c->modal.nModes);
    prepare_pencil(c, "mfh_modal_random");
    require_basis(c, "mfh_modal_random");
    const int m = c->modal.nModes;
    const int64_t n = c->modal.n, ld = c->modal.ld;
    const std::vector<double> lam = c->modal.lambda;
    if (correct) check_correctable(c, "mfh_modal_random");
    require(all_finite(f, (int64_t)nl * n), MFH_ERR_INVALID, "mfh_modal_random: a load has an entry that is not finite");
    hipStream_t s = c->stream;
    c->modalNote.clear();

    // ---- the loads: g = Phi^T f_a (m x nLoad) and, with a correction, one static solve per load that is not zero off the fixed variables and
    // r_a = u_a - sum_j phi_j g_ja / lambda_j in the two reserved columns
    ModalLoads L;
    std::vector<const double *> fLoad((size_t)nl);
    for (int a = 0; a < nl; ++a) fLoad[(size_t)a] = f + (size_t)a * n;
    prepare_modal_loads(c, "mfh_modal_random", L, nl, fLoad.data(), correct, P.rtol, P.maxit, info ? &info->staticSolves : nullptr, info ? &info->staticIterations : nullptr);
    const double *const B = c->modal.B.p;
    const std::vector<double> &g = L.g;
    const bool corr = L.corr;
    const int nb = L.nb;
    if (corr) modal_note(c, "static correction: " + std::to_string(L.staticSolves) + " solve(s) of K u = f, " + std::to_string(L.staticIts) + " iterations");
    else if (correct) modal_note(c, "static correction: every load is zero off the fixed variables, nothing to correct");

    // ---- the covariances of displacement, velocity and acceleration (host), and their factors
    auto tc = std::chrono::steady_clock::now();
    std::vector<double> Cq[3];
    for (auto &v : Cq) v.assign((size_t)nb * nb, 0.0);
    {
        const mfh_status st = mfh_modal_covariance(m, lam.data(), g.data(), nl, P.rayleighMass, P.rayleighStiff, P.lossFactor, modalDamping, nFreq, omega, weights, S, corr ? 1 : 0,
                                                   Cq[0].data(), Cq[1].data(), Cq[2].data());
        if (st != MFH_OK)
            throw Error(st, "mfh_modal_random: mfh_modal_covariance refused the input (omega = 0 with a zero eigenvalue, d_j = 0, a spectrum that is not Hermitian or has a "
                            "negative diagonal, an entry that is not finite, or sums that overflow)");
    }
    const double covarianceMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc).count();
    if (cov)
        for (int q = 0; q < 3; ++q) std::copy(Cq[q].begin(), Cq[q].end(), cov + (size_t)q * nb * nb);
    const bool need[3] = {rmsFields != nullptr || nProbe > 0, (rmsFields != nullptr && wantV) || nProbe > 0, (rmsFields != nullptr || nProbe > 0) && wantA};
    const bool fieldOf[3] = {rmsFields != nullptr, rmsFields != nullptr && wantV, rmsFields != nullptr && wantA};
    tc = std::chrono::steady_clock::now();
    Factor fac[3];
    for (int q = 0; q < 3; ++q)
        if (need[q]) fac[q] = factor_or_throw(nb, Cq[q].data(), P.tol, "mfh_modal_random");
    const double factorMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc).count();

    // ---- the passes: fields and probes (the same kernel on the gathered rows)
    DBuf<double> dBp, dOut, dPout;
    const int64_t ldp = ((int64_t)nProbe + 31) / 32 * 32;
    if (nProbe) { gather_probe_rows(B, ld, nb, probeVars, nProbe, dBp, ldp, s); dPout.alloc((size_t)nProbe); std::fill(probeRms, probeRms + (size_t)4 * nProbe, 0.0); }
    if (rmsFields) dOut.alloc((size_t)ld);
    EventTimer tsolve(s);
    int plane = 0;
    for (int q = 0; q < 3; ++q) {
        if (!need[q]) continue;
        k::SumsqPlan plan;
        plan.build(nb, fac[q].F.data(), nb, fac[q].rank, fac[q].piv.data(), k::MODAL_NP, s);
        if (fieldOf[q]) {
            plan.run(n, B, ld, true, dOut.p, s);
            MFH_HIP(hipMemcpyAsync(rmsFields + (size_t)plane * (size_t)n, dOut.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
            ++plane;
        }
        if (nProbe) {
            plan.run(nProbe, dBp.p, ldp, true, dPout.p, s);
            MFH_HIP(hipMemcpyAsync(probeRms + (size_t)q * nProbe, dPout.p, (size_t)nProbe * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        MFH_HIP(hipStreamSynchronize(s));
        if (info) { info->ranks[q] = fac[q].rank; info->passes[q] = plan.passes; info->truncation[q] = fac[q].truncation; }
    }
    const double solveMs = tsolve.stop();
    if (nProbe) {
        const double twoPi = 6.283185307179586;
        for (int p = 0; p < nProbe; ++p) probeRms[(size_t)3 * nProbe + p] = probeRms[p] > 0.0 ? probeRms[(size_t)nProbe + p] / (twoPi * probeRms[p]) : 0.0;
    }
    // ---- the response spectra of the probes: H_p S H_p^H on the gathered rows, host arithmetic on nProbe nb numbers per frequency
    if (probePsd) {
        std::vector<double> hb((size_t)ldp * nb);
        dBp.download(hb.data(), hb.size(), s);
        std::vector<Cplx> H((size_t)nb * nl), hp((size_t)nl);
        for (int k2 = 0; k2 < nFreq; ++k2) {
            const double w = omega[k2];
            for (int j = 0; j < m; ++j) {
                const Cplx di = modal_dinv(lam[(size_t)j], w, P.rayleighMass, P.rayleighStiff, P.lossFactor, modalDamping ? modalDamping[j] : 0.0);
                for (int a = 0; a < nl; ++a) H[(size_t)j * nl + a] = Cplx{g[(size_t)j * nl + a] * di.re, g[(size_t)j * nl + a] * di.im};
            }
            if (corr) {
                const Cplx iz = inv_zK(w, P.rayleighStiff, P.lossFactor);
                for (int a = 0; a < nl; ++a)
                    for (int b = 0; b < nl; ++b) H[(size_t)(m + a) * nl + b] = a == b ? iz : Cplx{0.0, 0.0};
            }
            const double *Sk = S + (size_t)k2 * nl * nl * 2;
            for (int p = 0; p < nProbe; ++p) {
                for (int a = 0; a < nl; ++a) {
                    Cplx acc{0.0, 0.0};
                    for (int j = 0; j < nb; ++j) { const double bj = hb[(size_t)j * ldp + p]; acc.re += bj * H[(size_t)j * nl + a].re; acc.im += bj * H[(size_t)j * nl + a].im; }
                    hp[(size_t)a] = acc;
                }
                double v = 0.0;
                for (int a = 0; a < nl; ++a)
                    for (int b = 0; b < nl; ++b) {       // Re(hp_a S_ab conj(hp_b))
                        const Cplx sab{Sk[(size_t)(a * nl + b) * 2], Sk[(size_t)(a * nl + b) * 2 + 1]};
                        const Cplx t{hp[(size_t)a].re * sab.re - hp[(size_t)a].im * sab.im, hp[(size_t)a].re * sab.im + hp[(size_t)a].im * sab.re};
                        v += t.re * hp[(size_t)b].re + t.im * hp[(size_t)b].im;
                    }
                probePsd[(size_t)p * nFreq + k2] = v;
            }
        }
    }
    if (info) {
        info->nb = nb;
        info->staticSolves = L.staticSolves; info->staticIterations = L.staticIts;
        info->covarianceMs = covarianceMs; info->factorMs = factorMs; info->solveMs = solveMs;
        info->note = c->modalNote.c_str();
    }
    MFH_CATCH(c)
}

// ---------------------------------------------------------------- modal stress recovery (docs/design/04_24_modal_stress.md)
}   // extern "C"

namespace {

// The stress passes of one covariance C = F F^T over the nb columns of B: the factor fields u_t = B F[:, t] in groups of planesPerPass <= 32 through
// k_modal_expand into `planes` (32 x ld doubles), then one launch of k_modal_stress_sumsq per group, which adds the squares of the group's corner
// stresses to dVm (and dComp unless null) and takes the roots on the last group. F: nb x rank, rows ldFh apart. rank 0: one launch with no plane, which
// writes zeros; B is not read.
struct StressRun {
    DBuf<double> planes, dC, partV, outV;
    DBuf<int64_t> partI, outI;
    int64_t corners = 0, flat = 0;
    void setup(const mfh_ctx *c, int64_t ld) {
        const HostMesh &m = c->mesh;
        corners = m.nElem * (m.deg == 1 ? 1 : m.dim + 1);
        flat = m.dim * (m.dim + 1) / 2;
        planes.alloc((size_t)ld * k::MODAL_NP_MAX);
        partV.alloc(k::PEAK_GRID_CAP); partI.alloc(k::PEAK_GRID_CAP);
        outV.alloc(1); outI.alloc(1);
    }
    int run(mfh_ctx *c, const double *B, int64_t n, int64_t ld, int nb, const double *F, int ldFh, int rank, int planesPerPass, int wantStress, bool root, double *dVm,
            double *dComp, hipStream_t s) {
        if (rank <= 0) {          // the kernel's own path: no plane, accumulators from 0.0 -- zeros, and neither B nor the scratch is read
            k::launch_modal_stress_sumsq(asm_args(c), c->dElemNodes.p, device_dof_map(c), c->tables.intGrad.data(), planes.p, ld, 0, wantStress, true, root, dVm, dComp, s);
            return 0;
        }
        const int ldc = rank + k::MODAL_NP_MAX;
        std::vector<double> hc((size_t)nb * ldc, 0.0);
        for (int j = 0; j < nb; ++j)
            for (int t = 0; t < rank; ++t) hc[(size_t)j * ldc + t] = F[(size_t)j * ldFh + t];
        dC.upload(hc, s);
        int passes = 0;
        for (int t0 = 0; t0 < rank; t0 += planesPerPass, ++passes) {
            const int np = std::min(planesPerPass, rank - t0);
            k::launch_modal_expand(n, B, ld, nb, dC.p + t0, ldc, np, k::MODAL_NP_MAX, planes.p, ld, s);
            k::launch_modal_stress_sumsq(asm_args(c), c->dElemNodes.p, device_dof_map(c), c->tables.intGrad.data(), planes.p, ld, np, wantStress, t0 == 0,
                                         root && t0 + np >= rank, dVm, dComp, s);
        }
        MFH_HIP(hipStreamSynchronize(s));      // hc and dC are this call's
        return passes;
    }
    // max / argmax of the n values of v by peak_before's order; synchronises
    void peak(const double *v, int64_t n, double *value, int64_t *index, hipStream_t s) {
        k::launch_peak_of_array(n, v, partV.p, partI.p, outV.p, outI.p, s);
        outV.download(value, 1, s);
        outI.download(index, 1, s);
        MFH_HIP(hipStreamSynchronize(s));
    }
};

void check_stress_outputs(const char *who, int32_t flags, const double *vm, const double *comp) {
    require_for((flags & ~(MFH_MODAL_STRESS_VON_MISES | MFH_MODAL_STRESS_COMPONENTS | MFH_MODAL_STRESS_STRAIN)) == 0, MFH_ERR_INVALID, who, "unknown stress flag");
    require_for((flags & (MFH_MODAL_STRESS_VON_MISES | MFH_MODAL_STRESS_COMPONENTS)) != 0, MFH_ERR_INVALID, who, "nothing asked for: MFH_MODAL_STRESS_VON_MISES | MFH_MODAL_STRESS_COMPONENTS");
    require_for(!(flags & MFH_MODAL_STRESS_VON_MISES) || vm, MFH_ERR_INVALID, who, "the von Mises output was requested but its pointer is null");
    require_for(!(flags & MFH_MODAL_STRESS_COMPONENTS) || comp, MFH_ERR_INVALID, who, "the components were requested but their pointer is null");
}

// the passes of nMat factors and their outputs; the von Mises sums are always formed (the peak is theirs)
void stress_outputs(mfh_ctx *c, int nb, const Factor *fac, int nMat, int32_t flags, double *rmsVonMises, double *rmsComponents, mfh_modal_stress_info *info) {
    hipStream_t s = c->stream;
    const int64_t n = c->modal.n, ld = c->modal.ld;
    StressRun R;
    R.setup(c, ld);
    DBuf<double> dVm, dComp;
    dVm.alloc((size_t)R.corners);
    const bool wantComp = (flags & MFH_MODAL_STRESS_COMPONENTS) != 0;
    if (wantComp) dComp.alloc((size_t)(R.corners * R.flat));
    for (int a = 0; a < nMat; ++a) {
        const int passes = R.run(c, c->modal.B.p, n, ld, nb, fac[a].F.data(), nb, fac[a].rank, k::MODAL_NP, (flags & MFH_MODAL_STRESS_STRAIN) ? 0 : 1, true, dVm.p,
                                 wantComp ? dComp.p : nullptr, s);
        double pv = 0.0;
        int64_t pi = 0;
        R.peak(dVm.p, R.corners, &pv, &pi, s);
        if (flags & MFH_MODAL_STRESS_VON_MISES) dVm.download(rmsVonMises + (size_t)a * (size_t)R.corners, (size_t)R.corners, s);
        if (wantComp) dComp.download(rmsComponents + (size_t)a * (size_t)(R.corners * R.flat), (size_t)(R.corners * R.flat), s);
        MFH_HIP(hipStreamSynchronize(s));
        if (info) {
            info->ranks[a] = fac[a].rank; info->passes[a] = passes; info->truncation[a] = fac[a].truncation;
            info->peakVonMises[a] = pv; info->peakCorner[a] = pi;
        }
    }
}

}   // namespace

extern "C" {

mfh_status mfh_modal_quadratic_stress(mfh_ctx *c, int32_t nMat, const double *C, double tol, int32_t flags, double *rmsVonMises, double *rmsComponents,
                                      mfh_modal_stress_info *info) {
    if (info) { *info = mfh_modal_stress_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_modal_quadratic_stress: null context");
    require(nMat >= 1 && nMat <= 4 && C != nullptr, MFH_ERR_INVALID, "mfh_modal_quadratic_stress: 1 <= nMat <= 4 matrices");
    require(!std::isnan(tol), MFH_ERR_INVALID, "mfh_modal_quadratic_stress: tol is not a number");
    check_stress_outputs("mfh_modal_quadratic_stress", flags, rmsVonMises, rmsComponents);
    prepare_pencil(c, "mfh_modal_quadratic_stress");
    require_basis(c, "mfh_modal_quadratic_stress");
    const int m = c->modal.nModes;
    c->modalNote.clear();
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<Factor> fac;
    for (int a = 0; a < nMat; ++a) fac.push_back(factor_or_throw(m, C + (size_t)a * m * m, tol, "mfh_modal_quadratic_stress"));
    const double factorMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    EventTimer tsolve(c->stream);
    stress_outputs(c, m, fac.data(), nMat, flags, rmsVonMises, rmsComponents, info);
    const double solveMs = tsolve.stop();
    if (info) { info->nb = m; info->factorMs = factorMs; info->solveMs = solveMs; info->note = c->modalNote.c_str(); }
    MFH_CATCH(c)
}

mfh_status mfh_modal_random_stress(mfh_ctx *c, const mfh_modal_random_params *prm, const double *omega, const double *weights, const double *modalDamping, const double *f,
                                   const double *S, int32_t stressFlags, double *rmsVonMises, double *rmsComponents, double *cov, mfh_modal_stress_info *info) {
    if (info) { *info = mfh_modal_stress_info{}; info->note = ""; }
    MFH_TRY(c)
    const char *who = "mfh_modal_random_stress";
    require(c != nullptr, MFH_ERR_INVALID, "mfh_modal_random_stress: null context");
    require(prm != nullptr, MFH_ERR_INVALID, "mfh_modal_random_stress: params is null");
    const mfh_modal_random_params P = *prm;
    require(P.nFreq >= 1 && P.maxit > 0, MFH_ERR_INVALID, "mfh_modal_random_stress: nFreq >= 1, maxit > 0");
    require(P.nLoad >= 1 && P.nLoad <= 8, MFH_ERR_INVALID, "mfh_modal_random_stress: 1 <= nLoad <= 8");
    check_damping(who, P.rayleighMass, P.rayleighStiff, P.lossFactor);
    require(P.rtol > 0.0 && P.rtol < 1.0, MFH_ERR_INVALID, "mfh_modal_random_stress: 0 < rtol < 1");
    require(!std::isnan(P.tol), MFH_ERR_INVALID, "mfh_modal_random_stress: tol is not a number");
    require((P.flags & ~(MFH_MODAL_RV_STATIC_CORRECTION | MFH_MODAL_RV_VELOCITY | MFH_MODAL_RV_ACCELERATION)) == 0, MFH_ERR_INVALID, "mfh_modal_random_stress: unknown flag");
    require((P.flags & (MFH_MODAL_RV_VELOCITY | MFH_MODAL_RV_ACCELERATION)) == 0, MFH_ERR_INVALID,
            "mfh_modal_random_stress: the stress of the displacement only: no velocity or acceleration flag");
    require(omega && f && S, MFH_ERR_INVALID, "mfh_modal_random_stress: omega, f and S are needed");
    check_stress_outputs(who, stressFlags, rmsVonMises, rmsComponents);
    const bool correct = (P.flags & MFH_MODAL_RV_STATIC_CORRECTION) != 0;
    require(!(correct && P.nLoad > 2), MFH_ERR_UNSUPPORTED, "mfh_modal_random_stress: the static correction has two reserved columns: at most two loads with it");
    const int nFreq = P.nFreq, nl = P.nLoad;
    for (int32_t k2 = 0; k2 < nFreq; ++k2) {
        require(std::isfinite(omega[k2]) && omega[k2] >= 0.0, MFH_ERR_INVALID, "mfh_modal_random_stress: a frequency is negative or not finite");
        require(k2 == 0 || omega[k2] > omega[k2 - 1], MFH_ERR_INVALID, "mfh_modal_random_stress: the frequencies are not ascending");
        require(omega[k2] > 0.0 || !c->fixedVars.empty(), MFH_ERR_INVALID, "mfh_modal_random_stress: omega = 0 needs fixed variables (K alone is singular)");
    }
    check_modal_damping(who, modalDamping, c->modal.nModes);
    prepare_pencil(c, who);
    require_basis(c, who);
    const int m = c->modal.nModes;
    const int64_t n = c->modal.n;
    const std::vector<double> lam = c->modal.lambda;
    if (correct) check_correctable(c, who);
    require(all_finite(f, (int64_t)nl * n), MFH_ERR_INVALID, "mfh_modal_random_stress: a load has an entry that is not finite");
    c->modalNote.clear();

    // ---- the loads, as mfh_modal_random sets them up
    ModalLoads L;
    std::vector<const double *> fLoad((size_t)nl);
    for (int a = 0; a < nl; ++a) fLoad[(size_t)a] = f + (size_t)a * n;
    prepare_modal_loads(c, who, L, nl, fLoad.data(), correct, P.rtol, P.maxit, info ? &info->staticSolves : nullptr, info ? &info->staticIterations : nullptr);
    const int nb = L.nb;
    if (L.corr) modal_note(c, "static correction: " + std::to_string(L.staticSolves) + " solve(s) of K u = f, " + std::to_string(L.staticIts) + " iterations");
    else if (correct) modal_note(c, "static correction: every load is zero off the fixed variables, nothing to correct");

    // ---- the covariance of the displacement coordinates (host) and its factor
    auto tc = std::chrono::steady_clock::now();
    std::vector<double> C0((size_t)nb * nb, 0.0);
    {
        const mfh_status st = mfh_modal_covariance(m, lam.data(), L.g.data(), nl, P.rayleighMass, P.rayleighStiff, P.lossFactor, modalDamping, nFreq, omega, weights, S,
                                                   L.corr ? 1 : 0, C0.data(), nullptr, nullptr);
        if (st != MFH_OK)
            throw Error(st, "mfh_modal_random_stress: mfh_modal_covariance refused the input (omega = 0 with a zero eigenvalue, d_j = 0, a spectrum that is not Hermitian or "
                            "has a negative diagonal, an entry that is not finite, or sums that overflow)");
    }
    const double covarianceMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc).count();
    tc = std::chrono::steady_clock::now();
    const Factor fac = factor_or_throw(nb, C0.data(), P.tol, who);
    const double factorMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc).count();
    if (cov) std::copy(C0.begin(), C0.end(), cov);

    EventTimer tsolve(c->stream);
    stress_outputs(c, nb, &fac, 1, stressFlags, rmsVonMises, rmsComponents, info);
    const double solveMs = tsolve.stop();
    if (info) {
        info->nb = nb;
        info->staticSolves = L.staticSolves; info->staticIterations = L.staticIts;
        info->covarianceMs = covarianceMs; info->factorMs = factorMs; info->solveMs = solveMs;
        info->note = c->modalNote.c_str();
    }
    MFH_CATCH(c)
}

// ---- hooks (include/meshfem_hip_extras.h)
mfh_status mfh_debug_modal_stress_sumsq(mfh_ctx *c, int32_t nPlanes, const double *U, int32_t planesPerPass, int32_t flags, int32_t sqrtFlag, double *vm, double *comp) {
    MFH_TRY(c)
    require(c && vm && nPlanes >= 0 && nPlanes <= 4096 && (nPlanes == 0 || U) && planesPerPass >= 0 && planesPerPass <= k::MODAL_NP_MAX && (sqrtFlag == 0 || sqrtFlag == 1) &&
                (flags & ~(MFH_MODAL_STRESS_VON_MISES | MFH_MODAL_STRESS_COMPONENTS | MFH_MODAL_STRESS_STRAIN)) == 0 && (!(flags & MFH_MODAL_STRESS_COMPONENTS) || comp),
            MFH_ERR_INVALID, "mfh_debug_modal_stress_sumsq: arguments");
    prepare_pencil(c, "mfh_debug_modal_stress_sumsq");
    ensure_geometry(c);
    hipStream_t s = c->stream;
    const int64_t n = (int64_t)c->bs() * c->nDoF, ld = (n + 31) / 32 * 32;
    const int per = planesPerPass ? planesPerPass : k::MODAL_NP;
    StressRun R;
    R.setup(c, ld);
    DBuf<double> dVm, dComp;
    dVm.alloc((size_t)R.corners);
    const bool wantComp = (flags & MFH_MODAL_STRESS_COMPONENTS) != 0;
    if (wantComp) dComp.alloc((size_t)(R.corners * R.flat));
    if (nPlanes == 0) {          // rank 0 as the drivers launch it, over a scratch of NaNs: the planes are not read
        MFH_HIP(hipMemsetAsync(R.planes.p, 0xFF, R.planes.n * sizeof(double), s));
        R.run(c, nullptr, n, ld, 0, nullptr, 0, 0, per, (flags & MFH_MODAL_STRESS_STRAIN) ? 0 : 1, sqrtFlag != 0, dVm.p, wantComp ? dComp.p : nullptr, s);
    }
    for (int t0 = 0; t0 < nPlanes; t0 += per) {
        const int np = std::min(per, nPlanes - t0);
        upload_columns(R.planes.p, ld, U + (size_t)t0 * (size_t)n, n, np, s);
        k::launch_modal_stress_sumsq(asm_args(c), c->dElemNodes.p, device_dof_map(c), c->tables.intGrad.data(), R.planes.p, ld, np, (flags & MFH_MODAL_STRESS_STRAIN) ? 0 : 1,
                                     t0 == 0, sqrtFlag != 0 && t0 + np >= nPlanes, dVm.p, wantComp ? dComp.p : nullptr, s);
    }
    dVm.download(vm, (size_t)R.corners, s);
    if (wantComp) dComp.download(comp, (size_t)(R.corners * R.flat), s);
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

mfh_status mfh_debug_peak_of_array(mfh_ctx *c, int64_t n, const double *v, double *value, int64_t *index) {
    MFH_TRY(c)
    require(c && v && value && index && n >= 1, MFH_ERR_INVALID, "mfh_debug_peak_of_array: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DBuf<double> d, partV, outV;
    DBuf<int64_t> partI, outI;
    d.alloc((size_t)n); partV.alloc(k::PEAK_GRID_CAP); partI.alloc(k::PEAK_GRID_CAP); outV.alloc(1); outI.alloc(1);
    upload(d.p, v, n, s);
    k::launch_peak_of_array(n, d.p, partV.p, partI.p, outV.p, outI.p, s);
    outV.download(value, 1, s);
    outI.download(index, 1, s);
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

// ms per repetition of one pass of k_modal_stress_sumsq over nPlanes <= 32 hashed planes (von Mises only) and of nPlanes launches of k_stress_measures (von
// Mises only) on the same planes, the two taking turns
mfh_status mfh_time_modal_stress(mfh_ctx *c, int32_t nPlanes, int32_t reps, double *stressMs, double *measuresMs) {
    MFH_TRY(c)
    require(c && stressMs && measuresMs && nPlanes >= 1 && nPlanes <= k::MODAL_NP_MAX && reps >= 1, MFH_ERR_INVALID, "mfh_time_modal_stress: arguments");
    prepare_pencil(c, "mfh_time_modal_stress");
    ensure_geometry(c);
    require(c->dofForNode.empty(), MFH_ERR_UNSUPPORTED, "mfh_time_modal_stress: contexts without a DoF map (k_stress_measures reads node-numbered planes)");
    hipStream_t s = c->stream;
    const int64_t n = (int64_t)c->bs() * c->nDoF, ld = (n + 31) / 32 * 32;
    StressRun R;
    R.setup(c, ld);
    DBuf<double> dVm, dVm1;
    dVm.alloc((size_t)R.corners); dVm1.alloc((size_t)R.corners);
    k::launch_fill_hash((int64_t)R.planes.n, R.planes.p, s);
    auto a = [&] { k::launch_modal_stress_sumsq(asm_args(c), c->dElemNodes.p, nullptr, c->tables.intGrad.data(), R.planes.p, ld, nPlanes, 1, true, true, dVm.p, nullptr, s); };
    auto b = [&] {
        for (int t = 0; t < nPlanes; ++t)
            k::launch_stress_measures(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), R.planes.p + (int64_t)t * ld, 1, 1, dVm1.p, nullptr, nullptr, s);
    };
    a(); b();          // warm-up
    MFH_HIP(hipStreamSynchronize(s));
    for (int r = 0; r < reps; ++r) {
        { EventTimer t(s); a(); stressMs[r] = t.stop(); }
        { EventTimer t(s); b(); measuresMs[r] = t.stop(); }
    }
    MFH_CATCH(c)
}

mfh_status mfh_debug_modal_sumsq(mfh_ctx *c, int64_t n, int32_t nb, const double *Bh, const double *Fh, int32_t rank, const int32_t *piv, int32_t planesPerPass,
                                 int32_t sqrtFlag, double *out) {
    MFH_TRY(c)
    require(c && out && n >= 1 && nb >= 1 && nb <= k::MODAL_MAXB && rank >= 0 && rank <= 4096 && (rank == 0 || (Bh && Fh)) && planesPerPass >= 0 &&
                planesPerPass <= k::MODAL_NP_MAX && (sqrtFlag == 0 || sqrtFlag == 1),
            MFH_ERR_INVALID, "mfh_debug_modal_sumsq: arguments");
    if (piv) {          // what a list leaves out has to be exactly zero from the pass's first column on
        require(rank <= nb, MFH_ERR_INVALID, "mfh_debug_modal_sumsq: a pivot list has at most nb entries");
        const int np = planesPerPass ? planesPerPass : k::MODAL_NP;
        for (int t = 0; t < rank; ++t) {
            require(piv[t] >= 0 && piv[t] < nb, MFH_ERR_INVALID, "mfh_debug_modal_sumsq: pivot out of range");
            for (int u = (t / np + 1) * np; u < rank; ++u) require(Fh[(size_t)piv[t] * rank + u] == 0.0, MFH_ERR_INVALID, "mfh_debug_modal_sumsq: a column the list leaves out has a non-zero coefficient");
        }
    }
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t ld = (n + 31) / 32 * 32;
    DBuf<double> b, o;
    o.alloc((size_t)ld);
    if (rank > 0) {
        b.alloc((size_t)ld * nb);
        b.zero(s);
        upload_columns(b.p, ld, Bh, n, nb, s);
    }
    k::SumsqPlan plan;
    plan.build(nb, Fh, rank, rank, piv, planesPerPass ? planesPerPass : k::MODAL_NP, s);
    plan.run(n, b.p, ld, sqrtFlag != 0, o.p, s);
    o.download(out, (size_t)n, s);
    MFH_CATCH(c)
}

// ms per repetition of one pass of k_modal_sumsq<NP> (all nb columns) and of one pass of k_modal_expand<NP> on the same hashed columns, the two taking
// turns; laterMs (or NULL): a second pass of a factor of rank 2 NP with pivots 0 .. NP - 1 -- nc = nb - NP columns and the accumulator read back
mfh_status mfh_time_modal_sumsq(mfh_ctx *c, int64_t n, int32_t nb, int32_t planesPerPass, int32_t reps, double *sumsqMs, double *expandMs, double *laterMs) {
    MFH_TRY(c)
    require(c && sumsqMs && expandMs && n >= 1 && reps >= 1 && nb >= 1 && nb <= k::MODAL_MAXB && (planesPerPass == 0 || planesPerPass == 8 || planesPerPass == 16 || planesPerPass == 32),
            MFH_ERR_INVALID, "mfh_time_modal_sumsq: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int np = planesPerPass ? planesPerPass : k::MODAL_NP;
    const int64_t ld = (n + 31) / 32 * 32;
    const int ldc = np + k::MODAL_NP_MAX;
    DBuf<double> b, cc, o, o1;
    b.alloc((size_t)ld * nb); o.alloc((size_t)ld * np); o1.alloc((size_t)ld); cc.alloc((size_t)nb * ldc);
    k::launch_fill_hash((int64_t)b.n, b.p, s);
    k::launch_fill_hash((int64_t)cc.n, cc.p, s);
    std::vector<double> hf((size_t)nb * np);
    for (size_t i = 0; i < hf.size(); ++i) hf[i] = 0.25 + (double)((i * 2654435761u) % 1024) / 1024.0;
    k::SumsqPlan plan;
    plan.build(nb, hf.data(), np, np, nullptr, np, s);
    k::SumsqPlan plan2;
    const bool later = laterMs != nullptr && nb > np;
    if (later) {          // rank 2 NP, lower trapezoidal in the first NP rows: the second pass leaves the columns 0 .. NP - 1 out
        std::vector<double> hf2((size_t)nb * 2 * np);
        std::vector<int32_t> piv((size_t)2 * np);
        for (int j = 0; j < nb; ++j)
            for (int t = 0; t < 2 * np; ++t) hf2[(size_t)j * 2 * np + t] = (j < np && t > j) ? 0.0 : hf[((size_t)j * np + t % np)];
        for (int t = 0; t < 2 * np; ++t) piv[(size_t)t] = t < nb ? t : nb - 1;
        plan2.build(nb, hf2.data(), 2 * np, 2 * np, piv.data(), np, s);
    }
    auto a = [&] { plan.run(n, b.p, ld, true, o1.p, s); };
    auto e = [&] { k::launch_modal_expand(n, b.p, ld, nb, cc.p, ldc, np, np, o.p, ld, s); };
    auto l = [&] { plan2.run(n, b.p, ld, false, o1.p, s, 1); };
    a(); e();          // warm-up
    if (later) l();
    MFH_HIP(hipStreamSynchronize(s));
    for (int r = 0; r < reps; ++r) {
        { EventTimer t(s); a(); sumsqMs[r] = t.stop(); }
        { EventTimer t(s); e(); expandMs[r] = t.stop(); }
        if (laterMs) laterMs[r] = 0.0;
        if (later) { EventTimer t(s); l(); laterMs[r] = t.stop(); }
    }
    MFH_CATCH(c)
}

mfh_status mfh_modal_basis_state(mfh_ctx *c, int32_t *nModes, int32_t *valid) {
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_modal_basis_state: null context");
    if (nModes) *nModes = c->modal.nModes;
    if (valid) {
        *valid = 0;
        if (c->modal.nModes > 0) {
            try { require_basis(c, "mfh_modal_basis_state"); *valid = 1; } catch (const Error &) {}
        }
    }
    MFH_CATCH(c)
}

// ---- hooks (include/meshfem_hip_extras.h)
mfh_status mfh_debug_modal_gram(mfh_ctx *c, int64_t n, int32_t na, int32_t nv, const double *A, const double *V, double *G) {
    MFH_TRY(c)
    require(c && A && V && G && n >= 1 && na >= 1 && na <= k::MODAL_MAXB && nv >= 1 && nv <= k::MG_TV, MFH_ERR_INVALID, "mfh_debug_modal_gram: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t ld = (n + 31) / 32 * 32;
    DBuf<double> a, v, part, g;
    a.alloc((size_t)ld * na); v.alloc((size_t)ld * nv); part.alloc((size_t)k::MG_GRID_CAP * na * nv); g.alloc((size_t)na * nv);
    upload_columns(a.p, ld, A, n, na, s);
    upload_columns(v.p, ld, V, n, nv, s);
    k::launch_modal_gram(n, a.p, ld, na, v.p, ld, nv, part.p, g.p, s);
    g.download(G, (size_t)na * nv, s);
    MFH_CATCH(c)
}
mfh_status mfh_debug_modal_expand(mfh_ctx *c, int64_t n, int32_t nb, const double *Bh, const double *Ch, int32_t nPlanes, int32_t planesPerPass, double *out) {
    MFH_TRY(c)
    require(c && Bh && Ch && out && n >= 1 && nb >= 1 && nb <= k::MODAL_MAXB && nPlanes >= 1 && nPlanes <= 4096 && planesPerPass >= 0 && planesPerPass <= k::MODAL_NP_MAX,
            MFH_ERR_INVALID, "mfh_debug_modal_expand: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t ld = (n + 31) / 32 * 32;
    const int ldc = nPlanes + k::MODAL_NP_MAX;
    DBuf<double> b, cc, o;
    b.alloc((size_t)ld * nb); o.alloc((size_t)nPlanes * (size_t)n);
    b.zero(s);
    upload_columns(b.p, ld, Bh, n, nb, s);
    std::vector<double> hc((size_t)nb * ldc, 0.0);
    for (int j = 0; j < nb; ++j)
        for (int p = 0; p < nPlanes; ++p) hc[(size_t)j * ldc + p] = Ch[(size_t)j * nPlanes + p];
    cc.upload(hc, s);
    k::launch_modal_expand(n, b.p, ld, nb, cc.p, ldc, nPlanes, planesPerPass ? planesPerPass : k::MODAL_NP, o.p, n, s);
    o.download(out, (size_t)nPlanes * (size_t)n, s);
    MFH_CATCH(c)
}

mfh_status mfh_time_modal_expand(mfh_ctx *c, int64_t n, int32_t nb, int32_t planesPerPass, int32_t reps, double *times) {
    MFH_TRY(c)
    require(c && times && n >= 1 && reps >= 1 && nb >= 1 && nb <= k::MODAL_MAXB && (planesPerPass == 0 || planesPerPass == 8 || planesPerPass == 16 || planesPerPass == 32),
            MFH_ERR_INVALID, "mfh_time_modal_expand: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int np = planesPerPass ? planesPerPass : k::MODAL_NP;
    const int64_t ld = (n + 31) / 32 * 32;
    const int ldc = np + k::MODAL_NP_MAX;
    DBuf<double> b, cc, o;
    b.alloc((size_t)ld * nb); o.alloc((size_t)ld * np); cc.alloc((size_t)nb * ldc);
    k::launch_fill_hash((int64_t)b.n, b.p, s);
    k::launch_fill_hash((int64_t)cc.n, cc.p, s);
    for (int r = 0; r < 2; ++r) k::launch_modal_expand(n, b.p, ld, nb, cc.p, ldc, np, np, o.p, ld, s);      // warm-up
    MFH_HIP(hipStreamSynchronize(s));
    for (int r = 0; r < reps; ++r) {
        EventTimer t(s);
        k::launch_modal_expand(n, b.p, ld, nb, cc.p, ldc, np, np, o.p, ld, s);
        times[r] = t.stop();
    }
    MFH_CATCH(c)
}

}   // extern "C"
