// Vibrational modes (mfh_modes, include/meshfem_hip.h; docs/design/04_12_modes.md): the smallest eigenpairs of K x = lambda M x by LOBPCG -- a host
// loop over device kernels. The reference's counterpart is smallestNonzeroGenEigenpairsPSDKnownKernel (Eigensolver.hh: shift-invert Lanczos over
// CHOLMOD); here K is never factored, the context's preconditioner (block-Jacobi / two-level / multigrid V-cycle) plays the part of the inverse.
//   block vectors   n x <= 24, the columns stored apart, ld = n rounded up to 32 doubles (the layout mg_precond_batch takes)
//   k_block_gram    G = A^T B: one wave per 6 x 8 tile of column pairs, the lanes take the 64 rows of a slab, tiles in registers, rows summed by
//                   wave reductions, one partial per workgroup; k_block_partial_sum adds the partials in workgroup order. No atomics.
//   k_block_update  Y1 = [A1 A2 A3] C1, Y2 = [A1 A2 A3] C2 (row-local, so outputs may be inputs): the lanes take rows, the coefficients are
//                   wave-uniform scalar loads. One launch serves the vectors and their K- and M-images (blockIdx.y).
//   k_block_residual  R = KX - MX diag(lambda) with the column norms of R and MX through the same two stages
//   k_deflate_gram / k_deflate_update  more modes than one block holds (mfh_modes_many; docs/design/04_19_many_modes.md): the projection of <= 24
//                   active columns against a deflation set of <= 262 contiguous locked columns that stays on the device -- G = (MQ)^T V from
//                   6 x 8 register tiles (groups of Q on blockIdx.x, slabs on blockIdx.y, k_block_partial_sum as second stage) and V -= Q C in
//                   place (C wave-uniform scalar loads, the row's sums in registers, Q streamed once). No atomics.
//   host            Cholesky-QR coefficients (chol_qr_factor), Rayleigh-Ritz (sym_gen_eig: Cholesky reduction + cyclic Jacobi, <= 72 x 72), locking,
//                   the loop. One loop serves the four entry points: ModesWork names the pencil (enum Pencil: vibration (K, rho M), buckling
//                   (Kg, K), prestressed (K + s Kg, rho M)) and its product members are the only code that switches on it; lobpcg_run(LoopIn,
//                   LoopOut) is the algorithm over the steps of struct Lobpcg (start_block, converged, new_directions, orthonormalise,
//                   rayleigh_ritz, return_columns). The entry points share ModesGuard, modes_prepare(ModesSetup), modes_fill_info and
//                   require_converged; mfh_modes_many adds many_orthonormalise_given, many_batches, many_full_residuals and many_sort.
//   k_spmv_kron_pair  prestressed vibration (mfh_modes_prestressed; docs/design/04_18_prestressed_modes.md): yA += s (Kg (x) I) x and
//                   yB = rho (M (x) I) x from ONE walk over the pattern -- k_spmv_kron_acc's chunks, every column index and x entry loaded once, two
//                   interleaved planes of LDS partials [dim][chunkSlots][2]. No atomics.
// FP64 throughout; two calls on one context with option "deterministic" return the same bits.
#include "mfh_pencil.hh"      // k_spmv_kron_acc (the accumulate pass of the tangent product and of the two-launch form of the pair product)
#include <deque>

namespace mfh { namespace k {

namespace {

constexpr int BLK_MAXC = 24;            // columns of a block vector
constexpr int GRAM_TP = 6, GRAM_TQ = 8; // column-pair tile of one wave
constexpr int GRAM_GRID_CAP = 512;      // workgroups of k_block_gram (= partials the second stage adds per entry)
constexpr int UPD_GRID_CAP = 2048;
constexpr int DEFL_MAXQ = 262;          // columns of a deflation set: 256 locked vectors and room for the 6 rigid modes
constexpr int DEFL_TQ = 6, DEFL_TV = 8; // column-pair tile of one wave of k_deflate_gram (Q x V); 8 x 8 spills at the 168 registers of 12 waves
constexpr int DEFL_WAVES = 12;          // waves of its workgroup: 12 / (tiles across V) tiles of Q, i.e. 24 / 36 / 72 columns of Q at <= 24 / 16 / 8 of V
constexpr int DEFL_GRID_CAP = 256;      // workgroups of k_deflate_gram along the rows (= partials the second stage adds per entry)

// the columns col[0 .. nc) of a block: column j at base + col[j] ld
struct BlockRef {
    const double *base;
    int64_t ld;
    int nc;
    unsigned char col[BLK_MAXC];
};

// partials[(blockIdx.x p + i) q + j] = sum over the rows of this workgroup's slabs of A_i B_j. Wave w of the workgroup owns the tile (w / ntq, w % ntq);
// the waves of a workgroup read the same slab at about the same time, so a column comes from HBM once and from the CU's L1 for the other tiles.
// Columns past the block's end are clamped to its last one (their sums are not written): the loop carries no branch.
__global__ void __launch_bounds__(768) k_block_gram(int64_t n, BlockRef A, BlockRef B, double *__restrict__ partials) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ntq = (B.nc + GRAM_TQ - 1) / GRAM_TQ;
    const int tp = wave / ntq, tq = wave - tp * ntq;
    const double *pa[GRAM_TP], *pb[GRAM_TQ];
#pragma unroll
    for (int i = 0; i < GRAM_TP; ++i) pa[i] = A.base + (int64_t)A.col[min(tp * GRAM_TP + i, A.nc - 1)] * A.ld;
#pragma unroll
    for (int j = 0; j < GRAM_TQ; ++j) pb[j] = B.base + (int64_t)B.col[min(tq * GRAM_TQ + j, B.nc - 1)] * B.ld;
    double acc[GRAM_TP][GRAM_TQ];
#pragma unroll
    for (int i = 0; i < GRAM_TP; ++i)
#pragma unroll
        for (int j = 0; j < GRAM_TQ; ++j) acc[i][j] = 0.0;
    const int64_t nSlab = (n + 63) >> 6;
    for (int64_t sl = blockIdx.x; sl < nSlab; sl += gridDim.x) {
        const int64_t row = (sl << 6) + lane;
        const bool ok = row < n;
        const int64_t r = ok ? row : 0;
        double a[GRAM_TP], b[GRAM_TQ];
#pragma unroll
        for (int i = 0; i < GRAM_TP; ++i) a[i] = pa[i][r];
#pragma unroll
        for (int j = 0; j < GRAM_TQ; ++j) b[j] = pb[j][r];
#pragma unroll
        for (int i = 0; i < GRAM_TP; ++i) a[i] = ok ? a[i] : 0.0;
#pragma unroll
        for (int j = 0; j < GRAM_TQ; ++j) b[j] = ok ? b[j] : 0.0;
#pragma unroll
        for (int i = 0; i < GRAM_TP; ++i)
#pragma unroll
            for (int j = 0; j < GRAM_TQ; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
    }
    double *out = partials + (int64_t)blockIdx.x * A.nc * B.nc;
#pragma unroll
    for (int i = 0; i < GRAM_TP; ++i)
#pragma unroll
        for (int j = 0; j < GRAM_TQ; ++j) {
            const double v = wave_sum(acc[i][j]);
            const int gi = tp * GRAM_TP + i, gj = tq * GRAM_TQ + j;
            if (lane == 0 && gi < A.nc && gj < B.nc) out[gi * B.nc + gj] = v;
        }
}

// out[e] = partials[0][e] + partials[1][e] + ... in that order (count entries per workgroup of the first stage)
__global__ void __launch_bounds__(256) k_block_partial_sum(int nPart, int count, const double *__restrict__ partials, double *__restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    double v = 0.0;
    for (int b = 0; b < nPart; ++b) v += partials[(int64_t)b * count + e];
    out[e] = v;
}

// One family of block vectors (the vectors themselves, their K-images or their M-images): three input blocks, two output blocks
struct UpdFamily {
    const double *in[3];
    double *out[2];
};
struct UpdArgs {
    int64_t n, ld;
    int nIn[3], nOut[2];
    int skip2;                            // output 2 takes the inputs from (flattened) index skip2 on
    int nFam;
    unsigned char colIn[3][BLK_MAXC], colOut[2][BLK_MAXC];
    UpdFamily fam[3];
};

// out1 = [in0 in1 in2] C1, out2 = [in0 in1 in2](skip2 ...) C2(skip2 ...) for the family blockIdx.y. C1 / C2: row-major, one row of BLK_MAXC doubles per
// input column (zero-padded): wave-uniform, read-only -> scalar loads, the products take them as scalar operands. A lane reads every input of its row
// before it writes any output, and rows do not interact: outputs may be inputs.
__global__ void __launch_bounds__(256) k_block_update(UpdArgs a, const double *__restrict__ C1, const double *__restrict__ C2) {
    const UpdFamily &F = a.fam[blockIdx.y];
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < a.n; row += (int64_t)gridDim.x * 256) {
        double y1[BLK_MAXC], y2[BLK_MAXC];
#pragma unroll
        for (int q = 0; q < BLK_MAXC; ++q) { y1[q] = 0.0; y2[q] = 0.0; }
        int jj = 0;
        for (int b = 0; b < 3; ++b) {
            const double *base = F.in[b];
            for (int j = 0; j < a.nIn[b]; ++j, ++jj) {
                const double v = base[(int64_t)a.colIn[b][j] * a.ld + row];
                const double *c1 = C1 + jj * BLK_MAXC;
#pragma unroll
                for (int q = 0; q < BLK_MAXC; ++q) y1[q] = fma(v, c1[q], y1[q]);
                if (C2 && jj >= a.skip2) {
                    const double *c2 = C2 + jj * BLK_MAXC;
#pragma unroll
                    for (int q = 0; q < BLK_MAXC; ++q) y2[q] = fma(v, c2[q], y2[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < BLK_MAXC; ++q)
            if (q < a.nOut[0]) F.out[0][(int64_t)a.colOut[0][q] * a.ld + row] = y1[q];
        if (C2) {
#pragma unroll
            for (int q = 0; q < BLK_MAXC; ++q)
                if (q < a.nOut[1]) F.out[1][(int64_t)a.colOut[1][q] * a.ld + row] = y2[q];
        }
    }
}

struct ResArgs {
    int64_t n, ld;
    int nc;
    unsigned char col[BLK_MAXC];
    double lam[BLK_MAXC];
    const double *KX, *MX;
    double *R;
};
// R_j = KX_j - lam_j MX_j for the listed columns; partials[blockIdx.x][2 j] = sum R_j^2, [2 j + 1] = sum MX_j^2 over the rows of the workgroup
// (wave reductions, the four waves added in wave order): the second stage is k_block_partial_sum
__global__ void __launch_bounds__(256) k_block_residual(ResArgs a, double *__restrict__ partials) {
    __shared__ double red[4][2 * BLK_MAXC];
    double rr[BLK_MAXC], mm[BLK_MAXC];
#pragma unroll
    for (int j = 0; j < BLK_MAXC; ++j) { rr[j] = 0.0; mm[j] = 0.0; }
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < a.n; row += (int64_t)gridDim.x * 256) {
#pragma unroll
        for (int j = 0; j < BLK_MAXC; ++j)
            if (j < a.nc) {
                const int64_t at = (int64_t)a.col[j] * a.ld + row;
                const double mx = a.MX[at], r = fma(-a.lam[j], mx, a.KX[at]);
                a.R[at] = r;
                rr[j] = fma(r, r, rr[j]);
                mm[j] = fma(mx, mx, mm[j]);
            }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < BLK_MAXC; ++j) {
        const double vr = wave_sum(rr[j]), vm = wave_sum(mm[j]);
        if (lane == 0) { red[wave][2 * j] = vr; red[wave][2 * j + 1] = vm; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * BLK_MAXC)
        partials[(int64_t)blockIdx.x * 2 * BLK_MAXC + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// ---- projection against a long deflation set (mfh_modes_many; docs/design/04_19_many_modes.md): Q and its image BQ are nq <= DEFL_MAXQ contiguous
// columns (column i at base + i ld), V the listed columns of a block.
// partials[(blockIdx.y nq + i) k + j] = sum over the rows of this workgroup's slabs of BQ_i V_j. blockIdx.x takes a group of qg columns of Q and
// blockIdx.y the slabs, so the row partition depends on n only; wave w of the workgroup owns the tile (w / ntv, w % ntv) of DEFL_TQ x DEFL_TV column
// pairs inside the group, as in k_block_gram. The waves of a workgroup walk the same slabs together: a column of Q is loaded once, a column of V
// once per group of Q -- and the groups of one slab set are neighbours in dispatch order, so they ask for the same slab of V at about the same time.
__global__ void __launch_bounds__(768) k_deflate_gram(int64_t n, const double *__restrict__ BQ, int64_t ldq, int nq, int qg, BlockRef V, double *__restrict__ partials) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ntv = (V.nc + DEFL_TV - 1) / DEFL_TV;
    const int tq = wave / ntv, tv = wave - tq * ntv;
    const int q0 = blockIdx.x * qg + tq * DEFL_TQ;
    if (q0 >= nq) return;                                   // (wave-uniform; the kernel has no barrier)
    const double *pa[DEFL_TQ], *pb[DEFL_TV];
#pragma unroll
    for (int i = 0; i < DEFL_TQ; ++i) pa[i] = BQ + (int64_t)min(q0 + i, nq - 1) * ldq;
#pragma unroll
    for (int j = 0; j < DEFL_TV; ++j) pb[j] = V.base + (int64_t)V.col[min(tv * DEFL_TV + j, V.nc - 1)] * V.ld;
    double acc[DEFL_TQ][DEFL_TV];
#pragma unroll
    for (int i = 0; i < DEFL_TQ; ++i)
#pragma unroll
        for (int j = 0; j < DEFL_TV; ++j) acc[i][j] = 0.0;
    const int64_t nSlab = (n + 63) >> 6;
    for (int64_t sl = blockIdx.y; sl < nSlab; sl += gridDim.y) {
        const int64_t row = (sl << 6) + lane;
        const bool ok = row < n;
        const int64_t r = ok ? row : 0;
        double a[DEFL_TQ], b[DEFL_TV];
#pragma unroll
        for (int i = 0; i < DEFL_TQ; ++i) a[i] = pa[i][r];
#pragma unroll
        for (int j = 0; j < DEFL_TV; ++j) b[j] = pb[j][r];
#pragma unroll
        for (int i = 0; i < DEFL_TQ; ++i) a[i] = ok ? a[i] : 0.0;
#pragma unroll
        for (int j = 0; j < DEFL_TV; ++j) b[j] = ok ? b[j] : 0.0;
#pragma unroll
        for (int i = 0; i < DEFL_TQ; ++i)
#pragma unroll
            for (int j = 0; j < DEFL_TV; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
    }
    double *out = partials + (int64_t)blockIdx.y * nq * V.nc;
#pragma unroll
    for (int i = 0; i < DEFL_TQ; ++i)
#pragma unroll
        for (int j = 0; j < DEFL_TV; ++j) {
            const double v = wave_sum(acc[i][j]);
            const int gi = q0 + i, gj = tv * DEFL_TV + j;
            if (lane == 0 && gi < nq && gj < V.nc) out[gi * V.nc + gj] = v;
        }
}

// V_j -= sum_i Q_i C[i][j] on the listed columns of V, in place. C: nq rows of BLK_MAXC doubles (zero-padded), wave-uniform and read-only -> scalar
// loads, as in k_block_update. A lane keeps the NC sums of its row in registers and streams the nq columns of Q once (four loads in flight);
// NC = the column count rounded up to 8, so a block that has shrunk to a few active columns does not pay for 24.
template <int NC>
__global__ void __launch_bounds__(256) k_deflate_update(int64_t n, const double *__restrict__ Q, int64_t ldq, int nq, const double *__restrict__ C, BlockRef V) {
    double *vb = const_cast<double *>(V.base);
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n; row += (int64_t)gridDim.x * 256) {
        double s[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) s[j] = 0.0;
        const double *q = Q + row;
        int i = 0;
        for (; i + 4 <= nq; i += 4) {
            const double q0 = q[(int64_t)i * ldq], q1 = q[(int64_t)(i + 1) * ldq], q2 = q[(int64_t)(i + 2) * ldq], q3 = q[(int64_t)(i + 3) * ldq];
            const double *c = C + i * BLK_MAXC;
#pragma unroll
            for (int j = 0; j < NC; ++j) s[j] = fma(q0, c[j], s[j]);
#pragma unroll
            for (int j = 0; j < NC; ++j) s[j] = fma(q1, c[BLK_MAXC + j], s[j]);
#pragma unroll
            for (int j = 0; j < NC; ++j) s[j] = fma(q2, c[2 * BLK_MAXC + j], s[j]);
#pragma unroll
            for (int j = 0; j < NC; ++j) s[j] = fma(q3, c[3 * BLK_MAXC + j], s[j]);
        }
        for (; i < nq; ++i) {
            const double q0 = q[(int64_t)i * ldq];
            const double *c = C + i * BLK_MAXC;
#pragma unroll
            for (int j = 0; j < NC; ++j) s[j] = fma(q0, c[j], s[j]);
        }
#pragma unroll
        for (int j = 0; j < NC; ++j)
            if (j < V.nc) {
                const int64_t at = (int64_t)V.col[j] * V.ld + row;
                vb[at] = vb[at] - s[j];
            }
    }
}

// flags a prestress entry that is not finite (the lanes store the flag: no atomic)
__global__ void __launch_bounds__(256) k_prestress_finite(int64_t n, const double *__restrict__ sigma, int *__restrict__ flag) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const double v = sigma[e];
        if (!(v - v == 0.0)) flag[0] = 1;
    }
}

// The two one-double-per-block products of the prestressed pencil from ONE walk over the pattern (rowPtr, colIdx) of a (a.vals is not read):
//     yA[N i + c] = yA[N i + c] + sG sum_j g_ij x[N j + c]      (g = the geometric stiffness buffer; yA holds K x on entry)
//     yB[N i + c] =               rho sum_j m_ij x[N j + c]      (m = the mass buffer)
// both zero on the fixed rows where a mask is given. The chunk walk and the tiling are k_spmv_kron_acc's; every column index and every x entry is
// loaded once and multiplied by both stored values into two planes of LDS partials, [N][chunkSlots] pairs {g x, m x} (the pattern of
// k_spmv_kron_cacc; the planes interleaved, so that a slot's pair is one 16-byte store and one 16-byte load). Then one lane per scalar row adds
// the row's partials of both planes in slot order: the sums, and the two roundings of yA + sG sum, are those of k_spmv_kron_acc and k_spmv_kron,
// so this kernel and the two-launch form give the same bits. No atomics.
template <int N>
__global__ void __launch_bounds__(256) k_spmv_kron_pair(SpmvArgs a, const double *__restrict__ gVals, const double *__restrict__ mVals, double sG, double rho,
                                                       const double *__restrict__ x, double *yA, double *__restrict__ yB) {
    extern __shared__ __attribute__((aligned(16))) double part[];  // [N][chunkSlots][2] + 16
    double2 *pair = reinterpret_cast<double2 *>(part);
    const int CS = a.chunkSlots;
    for (int64_t chunk = blockIdx.x; chunk < a.nChunk; chunk += gridDim.x) {
        const int r0 = a.chunkRow[chunk], r1 = a.chunkRow[chunk + 1];
        const int s0 = a.rowPtr[r0];
        const int ns = a.rowPtr[r1] - s0;
        for (int t = threadIdx.x; t < ns; t += 256) {
            const int64_t s = (int64_t)s0 + t;
            const int64_t col = a.colIdx[s];
            const int64_t at = tiled_index(s, 0, 1);
            const double g = gVals[at], m = mVals[at];
#pragma unroll
            for (int c = 0; c < N; ++c) {
                const double xv = x[col * N + c];
                pair[c * CS + t] = make_double2(g * xv, m * xv);
            }
        }
        __syncthreads();
        const int nscalar = (r1 - r0) * N;
        for (int idx = threadIdx.x; idx < nscalar; idx += 256) {
            const int rl = idx / N, c = idx - rl * N;
            const int64_t r = r0 + rl;
            const int b = a.rowPtr[r] - s0, e = a.rowPtr[r + 1] - s0;
            const double2 *pp = pair + c * CS;
            double vg = 0, vm = 0;
            for (int t = b; t < e; ++t) {
                const double2 p = pp[t];
                vg += p.x;
                vm += p.y;
            }
            const int64_t gi = r * N + c;
            {
#pragma clang fp contract(off)                                          // (the product rounded before the sum, as the two-launch form rounds it)
                vg = sG * vg;
                vg = yA[gi] + vg;
                vm = rho * vm;
            }
            if (a.fixedMask && a.fixedMask[gi]) { vg = 0.0; vm = 0.0; }
            yA[gi] = vg;
            yB[gi] = vm;
        }
        __syncthreads();
    }
}

// yA += sG Kg x and yB = rho M x (pat: the pattern, chunks and mask of mass_spmv_args). One pass (k_spmv_kron_pair) where its LDS fits and twoPass is
// not set; else the existing kernels in two launches: k_spmv_kron_acc on the geometric buffer, k_spmv_kron on the mass buffer and the density
// scaling. The grids depend on the pattern alone. true: the single pass ran.
bool launch_spmv_kron_pair(const SpmvArgs &pat, const double *gVals, const double *mVals, double sG, double rho, const double *x, double *yA, double *yB,
                           int64_t n, bool twoPass, hipStream_t s) {
    if (pat.nChunk <= 0) return false;
    if (pat.dim != 2 && pat.dim != 3) throw mfh::Error(MFH_ERR_UNSUPPORTED, "k_spmv_kron_pair: 2D / 3D only");
    const size_t lds = ((size_t)2 * pat.dim * pat.chunkSlots + 16) * sizeof(double);
    if (!twoPass && lds <= HARM_LDS_MAX) {
        const int grid = (int)std::min<int64_t>(pat.nChunk, DYN_GRID_CAP);
        with_dim(pat.dim, [&](auto D) { launch_k(k_spmv_kron_pair<D()>, dim3(grid), dim3(256), lds, s, pat, gVals, mVals, sG, rho, x, yA, yB); });
        CHECK_LAUNCH();
        return true;
    }
    SpmvArgs a = pat;
    a.vals = gVals;
    launch_spmv_kron_acc(a, true, 1.0, sG, x, yA, nullptr, DynGate{nullptr, 0, nullptr}, s);
    a.vals = mVals;
    launch_spmv(a, x, yB, nullptr, s);
    if (rho != 1.0) launch_axpby(n, 0.0, yB, rho, yB, s);
    return false;
}

int gram_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 63) / 64, GRAM_GRID_CAP)); }

// G (device, p x q row-major) = A^T B; partials: scratch of GRAM_GRID_CAP * 576 doubles
void launch_block_gram(int64_t n, const BlockRef &A, const BlockRef &B, double *partials, double *G, hipStream_t s) {
    const int waves = ((A.nc + GRAM_TP - 1) / GRAM_TP) * ((B.nc + GRAM_TQ - 1) / GRAM_TQ);
    const int grid = gram_grid(n), count = A.nc * B.nc;
    hipLaunchKernelGGL(k_block_gram, dim3(grid), dim3(64 * waves), 0, s, n, A, B, partials);
    hipLaunchKernelGGL(k_block_partial_sum, dim3((count + 255) / 256), dim3(256), 0, s, grid, count, (const double *)partials, G);
    CHECK_LAUNCH();
}

void launch_block_update(const UpdArgs &a, const double *C1, const double *C2, hipStream_t s) {
    hipLaunchKernelGGL(k_block_update, dim3(grid_for(a.n, UPD_GRID_CAP), a.nFam), dim3(256), 0, s, a, C1, C2);
    CHECK_LAUNCH();
}

// norms (device, 2 BLK_MAXC doubles): [2 j] = ||R_j||^2, [2 j + 1] = ||MX_j||^2; partials: scratch of UPD_GRID_CAP * 48 doubles
void launch_block_residual(const ResArgs &a, double *partials, double *norms, hipStream_t s) {
    const int grid = grid_for(a.n, UPD_GRID_CAP);
    hipLaunchKernelGGL(k_block_residual, dim3(grid), dim3(256), 0, s, a, partials);
    hipLaunchKernelGGL(k_block_partial_sum, dim3(1), dim3(256), 0, s, grid, 2 * BLK_MAXC, (const double *)partials, norms);
    CHECK_LAUNCH();
}

int deflate_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 63) / 64, DEFL_GRID_CAP)); }

// G (device, nq x V.nc row-major) = BQ^T V; partials: scratch of DEFL_GRID_CAP * DEFL_MAXQ * BLK_MAXC doubles
void launch_deflate_gram(int64_t n, const double *BQ, int64_t ldq, int nq, const BlockRef &V, double *partials, double *G, hipStream_t s) {
    const int ntv = (V.nc + DEFL_TV - 1) / DEFL_TV, qg = DEFL_TQ * (DEFL_WAVES / ntv), ntq = (std::min(nq, qg) + DEFL_TQ - 1) / DEFL_TQ;
    const int grid = deflate_grid(n), count = nq * V.nc;
    hipLaunchKernelGGL(k_deflate_gram, dim3((nq + qg - 1) / qg, grid), dim3(64 * ntq * ntv), 0, s, n, BQ, ldq, nq, qg, V, partials);
    hipLaunchKernelGGL(k_block_partial_sum, dim3((count + 255) / 256), dim3(256), 0, s, grid, count, (const double *)partials, G);
    CHECK_LAUNCH();
}

// V (listed columns) -= Q C; C: device, nq rows of BLK_MAXC doubles
void launch_deflate_update(int64_t n, const double *Q, int64_t ldq, int nq, const double *C, const BlockRef &V, hipStream_t s) {
    const dim3 grid(grid_for(n, UPD_GRID_CAP)), block(256);
    if (V.nc <= 8) hipLaunchKernelGGL(k_deflate_update<8>, grid, block, 0, s, n, Q, ldq, nq, C, V);
    else if (V.nc <= 16) hipLaunchKernelGGL(k_deflate_update<16>, grid, block, 0, s, n, Q, ldq, nq, C, V);
    else hipLaunchKernelGGL(k_deflate_update<BLK_MAXC>, grid, block, 0, s, n, Q, ldq, nq, C, V);
    CHECK_LAUNCH();
}

}   // namespace

void launch_prestress_finite(int64_t n, const double *sigma, int *flag, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_prestress_finite, dim3(grid_for(n)), dim3(256), 0, s, n, sigma, flag);
    CHECK_LAUNCH();
}
}}   // namespace mfh::k

using namespace mfh;
using namespace mfhi;
using k::BlockRef;
using k::BLK_MAXC;

namespace {

constexpr int RR_MAX = 72;              // largest Rayleigh-Ritz problem: three blocks of 24
// the product form of the prestressed loop: k_spmv_kron_pair (true) or the two launches it replaces; settled by measurement (mfh_time_kron_pair,
// profiles/r14_prestressed_modes.md: at 60^3 quadratic tets the single pass takes 1.01 to 1.03 x the two launches at density 1). Both forms give the same bits.
constexpr bool PAIR_FUSED_DEFAULT = false;

// All eigenpairs of A v = w B v, A symmetric, B symmetric positive definite (null: the identity), n x n row-major, upper triangles read. Cholesky
// B = L L^T, C = L^-1 A L^-T, cyclic Jacobi on C (rotations of Rutishauser's form), V = L^-T Q. w ascending. false: B not positive definite.
bool sym_gen_eig(int n, const double *A, const double *B, double *w, double *V) {
    const size_t N = (size_t)n;
    std::vector<double> L(N * N, 0.0), Cm(N * N), Q(N * N, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Cm[i * N + j] = i <= j ? A[i * N + j] : A[j * N + i];
    if (B) {
        for (int j = 0; j < n; ++j) {
            double d = B[j * N + j];
            for (int q = 0; q < j; ++q) d -= L[j * N + q] * L[j * N + q];
            if (!(d > 0.0)) return false;
            const double ljj = std::sqrt(d);
            L[j * N + j] = ljj;
            for (int i = j + 1; i < n; ++i) {
                double v = B[j * N + i];
                for (int q = 0; q < j; ++q) v -= L[i * N + q] * L[j * N + q];
                L[i * N + j] = v / ljj;
            }
        }
        // T = L^-1 A (columns by forward substitution), then C = L^-1 T^T
        for (int pass = 0; pass < 2; ++pass) {
            for (int c = 0; c < n; ++c)
                for (int i = 0; i < n; ++i) {
                    double v = Cm[i * N + c];
                    for (int q = 0; q < i; ++q) v -= L[i * N + q] * Cm[q * N + c];
                    Cm[i * N + c] = v / L[i * N + i];
                }
            for (int i = 0; i < n; ++i)
                for (int j = i + 1; j < n; ++j) std::swap(Cm[i * N + j], Cm[j * N + i]);
        }
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) Cm[i * N + j] = Cm[j * N + i] = 0.5 * (Cm[i * N + j] + Cm[j * N + i]);
    }
    for (int i = 0; i < n; ++i) Q[i * N + i] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < n; ++i) {
            diag += Cm[i * N + i] * Cm[i * N + i];
            for (int j = i + 1; j < n; ++j) off += Cm[i * N + j] * Cm[i * N + j];
        }
        if (off == 0.0 || off <= 1e-34 * diag) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = Cm[p * N + q];
                if (apq == 0.0) continue;
                const double app = Cm[p * N + p], aqq = Cm[q * N + q];
                if (std::fabs(apq) <= 1e-300 || (sweep > 3 && std::fabs(apq) <= 2.2e-16 * 1e-4 * std::min(std::fabs(app), std::fabs(aqq)))) {
                    if (sweep > 3) { Cm[p * N + q] = Cm[q * N + p] = 0.0; }
                    continue;
                }
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs, tau = sn / (1.0 + cs);
                Cm[p * N + p] = app - t * apq;
                Cm[q * N + q] = aqq + t * apq;
                Cm[p * N + q] = Cm[q * N + p] = 0.0;
                for (int r = 0; r < n; ++r) {
                    if (r != p && r != q) {
                        const double arp = Cm[r * N + p], arq = Cm[r * N + q];
                        Cm[r * N + p] = Cm[p * N + r] = arp - sn * (arq + tau * arp);
                        Cm[r * N + q] = Cm[q * N + r] = arq + sn * (arp - tau * arq);
                    }
                    const double vrp = Q[r * N + p], vrq = Q[r * N + q];
                    Q[r * N + p] = vrp - sn * (vrq + tau * vrp);
                    Q[r * N + q] = vrq + sn * (vrp - tau * vrq);
                }
            }
    }
    std::vector<int> order(N);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return Cm[x * N + x] < Cm[y * N + y]; });
    for (int k2 = 0; k2 < n; ++k2) {
        const int src = order[k2];
        w[k2] = Cm[src * N + src];
        // column k2 of V = L^-T q (back substitution)
        for (int i = n - 1; i >= 0; --i) {
            double v = Q[i * N + src];
            if (B) {
                for (int q = i + 1; q < n; ++q) v -= L[q * N + i] * V[q * N + k2];
                v /= L[i * N + i];
            }
            V[i * N + k2] = v;
        }
    }
    return true;
}

// Upper-triangular U with (S U)^T M (S U) = I from the Gram matrix G = S^T M S (k x k row-major, symmetric): Cholesky of D^-1/2 G D^-1/2 with
// D = diag G, U = D^-1/2 L^-T. A pivot of the scaled matrix at or below `floor` (or a non-positive diagonal entry) fails: its index is returned
// (-1: success). U row-major k x k.
int chol_qr_factor(int k, const std::vector<double> &G, double floor, std::vector<double> &U) {
    const size_t K = (size_t)k;
    std::vector<double> L(K * K, 0.0), sc(K);
    for (int i = 0; i < k; ++i) {
        if (!(G[i * K + i] > 0.0) || !std::isfinite(G[i * K + i])) return i;
        sc[i] = 1.0 / std::sqrt(G[i * K + i]);
    }
    for (int j = 0; j < k; ++j) {
        double d = 1.0;
        for (int q = 0; q < j; ++q) d -= L[j * K + q] * L[j * K + q];
        if (!(d > floor)) return j;
        const double ljj = std::sqrt(d);
        L[j * K + j] = ljj;
        for (int i = j + 1; i < k; ++i) {
            double v = 0.5 * (G[i * K + j] + G[j * K + i]) * sc[i] * sc[j];
            for (int q = 0; q < j; ++q) v -= L[i * K + q] * L[j * K + q];
            L[i * K + j] = v / ljj;
        }
    }
    // U = D^-1/2 L^-T: column c of L^-T by back substitution on L^T
    U.assign(K * K, 0.0);
    for (int c = 0; c < k; ++c) {
        for (int i = c; i >= 0; --i) {
            double v = i == c ? 1.0 : 0.0;
            for (int q = i + 1; q <= c; ++q) v -= L[q * K + i] * U[q * K + c];
            U[i * K + c] = v / L[i * K + i];
        }
    }
    for (int i = 0; i < k; ++i)
        for (int c = i; c < k; ++c) U[i * K + c] *= sc[i];
    return -1;
}

// Rigid motions that the fixed variables leave free: the candidates (translations; rotations unless a DoF map identifies nodes) restricted to the
// fixed variables, as the constrained solve counts them (sim_solve_impl)
int free_rigid_motions(const mfh_ctx *c) {
    const HostMesh &m = c->mesh;
    const int d = m.dim;
    const bool periodic = !c->dofForNode.empty();
    const int nc = periodic ? d : (d == 3 ? 6 : 3);
    if (c->fixedVars.empty()) return nc;
    std::vector<int32_t> nodeOfDof;
    if (periodic) {
        nodeOfDof.assign((size_t)c->nDoF, -1);
        for (int64_t nd = m.nNode - 1; nd >= 0; --nd) nodeOfDof[(size_t)c->dofForNode[(size_t)nd]] = (int32_t)nd;
    }
    double cen[3] = {0, 0, 0}, ext = 0;
    {
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        for (int64_t nd = 0; nd < m.nNode; ++nd)
            for (int a = 0; a < d; ++a) { lo[a] = std::min(lo[a], m.nodePos[(size_t)nd * d + a]); hi[a] = std::max(hi[a], m.nodePos[(size_t)nd * d + a]); }
        for (int a = 0; a < d; ++a) { cen[a] = 0.5 * (lo[a] + hi[a]); ext = std::max(ext, hi[a] - lo[a]); }
        if (!(ext > 0)) ext = 1.0;
    }
    std::vector<double> G((size_t)nc * nc, 0.0);
    for (int64_t fv : c->fixedVars) {
        const int64_t dof = fv / d;
        const int comp = (int)(fv % d);
        const int64_t nd = periodic ? nodeOfDof[(size_t)dof] : dof;
        double x[3] = {0, 0, 0};
        for (int a = 0; a < d; ++a) x[a] = (m.nodePos[(size_t)nd * d + a] - cen[a]) / ext;
        double z[6] = {0, 0, 0, 0, 0, 0};
        z[comp] = 1.0;
        if (!periodic) {
            if (d == 3) {
                const double rot[3][3] = {{0, -x[2], x[1]}, {x[2], 0, -x[0]}, {-x[1], x[0], 0}};
                for (int r = 0; r < 3; ++r) z[3 + r] = rot[r][comp];
            } else
                z[2] = comp == 0 ? -x[1] : x[0];
        }
        for (int a = 0; a < nc; ++a)
            for (int b = 0; b < nc; ++b) G[(size_t)a * nc + b] += z[a] * z[b];
    }
    std::vector<double> w((size_t)nc), V((size_t)nc * nc);
    sym_gen_eig(nc, G.data(), nullptr, w.data(), V.data());
    int q = 0;
    for (int e = 0; e < nc; ++e)
        if (w[e] <= 1e-12 * std::max(w[nc - 1], 1e-300)) ++q;
    return q;
}

// The pencil (A, B) the loop works on; only the product members of ModesWork look at it
enum class Pencil {
    Vibration,                         // (K, density M): mfh_modes, mfh_modes_many
    Buckling,                          // (Kg, K), A indefinite: mfh_buckling
    Prestressed                        // (K + loadFactor Kg, density M), A indefinite beyond the critical load: mfh_modes_prestressed
};

struct ModesWork {
    mfh_ctx *c;
    hipStream_t s;
    int d, m;                          // variables per DoF, block size
    int64_t n, ld;
    double density = 1.0;
    bool masked;
    Pencil pencil = Pencil::Vibration;
    double loadFactor = 0.0;
    bool pairTwoPass = !PAIR_FUSED_DEFAULT;   // the product form of apply_AB (launch_spmv_kron_pair)
    const char *who = "mfh_modes";     // the entry point, for messages
    DBuf<double> vec, zvec, gramPart, resPart, small, coef;
    DBuf<double> deflPart, deflG, deflC;       // deflation set (mfh_modes_many): partials and Gram matrix of k_deflate_gram, coefficients of k_deflate_update
    double *X, *W, *P, *KX, *KW, *KP, *MX, *MW, *MP, *R;
    double *Z = nullptr, *KZ = nullptr, *MZ = nullptr;
    int nz = 0;
    size_t smallUsed = 0, coefUsed = 0;
    std::deque<std::vector<double>> staged;    // host sources of asynchronous uploads, alive until the next synchronisation
    bool useMG = false, useTL = false;
    // per-phase device time (scripts/probe_modes.py: env MFH_MODES_TIMING=1 puts a synchronisation at every phase boundary)
    bool timing = false;
    double tPhase[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // K products, M products, preconditioner, Gram, update, residual, host Rayleigh-Ritz incl. its synchronisation, deflation (both kernels, the coefficients' host trip)
    double tMark = 0;

    void lap(int phase) {
        if (!timing) return;
        MFH_HIP(hipStreamSynchronize(s));
        const double t = now_ms();
        if (phase >= 0) tPhase[phase] += t - tMark;
        tMark = t;
    }
    BlockRef ref(const double *base, const std::vector<int> &cols) const {
        BlockRef r{};
        r.base = base; r.ld = ld; r.nc = (int)cols.size();
        for (size_t j = 0; j < cols.size(); ++j) r.col[j] = (unsigned char)cols[j];
        return r;
    }
    void sync() {
        MFH_HIP(hipStreamSynchronize(s));
        staged.clear();
        smallUsed = 0;
        coefUsed = 0;
    }
    double *small_slot(size_t count) {
        need(smallUsed + count <= small.n, MFH_ERR_STATE, "Gram staging overflow");
        double *p = small.p + smallUsed;
        smallUsed += count;
        return p;
    }
    // device G slot = A^T B
    double *gram(const BlockRef &A, const BlockRef &B) {
        double *G = small_slot((size_t)A.nc * B.nc);
        k::launch_block_gram(n, A, B, gramPart.p, G, s);
        return G;
    }
    const double *upload_coef(std::vector<double> &&h) {
        need(coefUsed + h.size() <= coef.n, MFH_ERR_STATE, "coefficient staging overflow");
        staged.push_back(std::move(h));
        double *p = coef.p + coefUsed;
        coefUsed += staged.back().size();
        MFH_HIP(hipMemcpyAsync(p, staged.back().data(), staged.back().size() * sizeof(double), hipMemcpyHostToDevice, s));
        return p;
    }
    // The products of the pencil (A, B). In the loop the blocks named K* hold the A-images and the blocks named M* the B-images; B carries the
    // inner product, and the preconditioner approximates K^-1 in all three pencils. These members are the only code that switches on the kind.
    void apply_A(const double *x, double *y) {
        if (pencil == Pencil::Buckling) { k::launch_spmv(geom_spmv_args(c, masked), x, y, nullptr, s); return; }
        apply_operator(c, masked, x, y, nullptr);
        if (pencil == Pencil::Prestressed) k::launch_spmv_kron_acc(geom_spmv_args(c, masked), true, 1.0, loadFactor, x, y, nullptr, k::DynGate{nullptr, 0, nullptr}, s);
    }
    void apply_B(const double *x, double *y) {
        if (pencil == Pencil::Buckling) { apply_operator(c, masked, x, y, nullptr); return; }
        k::launch_spmv(mass_spmv_args(c, masked), x, y, nullptr, s);
        if (density != 1.0) k::launch_axpby(n, 0.0, y, density, y, s);      // the buffer holds density 1
    }
    // both images of one column of the prestressed pencil: K x into yA, then Kg's and M's parts from one walk over the pattern
    void apply_AB(const double *x, double *yA, double *yB, bool book) {
        apply_operator(c, masked, x, yA, nullptr);
        if (book) lap(0);
        k::launch_spmv_kron_pair(mass_spmv_args(c, masked), c->dGeomVals.p, c->dMassVals.p, loadFactor, density, x, yA, yB, n, pairTwoPass, s);
        if (book) lap(1);
    }
    // AV and BV = the images of the listed columns of V: all A-products, then all B-products; the prestressed pencil column by column through
    // apply_AB. book: under MFH_MODES_TIMING the A-products (of the prestressed pencil: K's) go to phase 0 and the others to phase 1.
    void apply_images(double *V, double *AV, double *BV, const std::vector<int> &cols, bool book) {
        if (pencil == Pencil::Prestressed) {
            for (int j : cols) apply_AB(col(V, j), col(AV, j), col(BV, j), book);
            return;
        }
        for (int j : cols) apply_A(col(V, j), col(AV, j));
        if (book) lap(0);
        for (int j : cols) apply_B(col(V, j), col(BV, j));
        if (book) lap(1);
    }
    // B is ill-conditioned where the mass matrix is not (B = K): the B-images carried through hundreds of block updates have drifted from K X by
    // far more than M X ever does (X K X^T - I of 3e-12 after 200 block-Jacobi iterations at cond 7e4), so the returned columns take theirs afresh
    bool recompute_returned_B() const { return pencil == Pencil::Buckling; }
    // the three families of the basis [X W P]: the vectors (0), their A-images (1), their B-images (2)
    double *block(int fam, int b) const {
        double *const t[3][3] = {{X, W, P}, {KX, KW, KP}, {MX, MW, MP}};
        return t[fam][b];
    }
    void need(bool cond, mfh_status code, const char *what) const { if (!cond) throw fail(code, what); }
    Error fail(mfh_status code, const char *what) const { return Error(code, std::string(who) + ": " + what); }
    void precond(const double *r, double *z) {
        if (useMG) mg_precond(c, r, z, nullptr, -1, nullptr);
        else if (useTL) tl_precond(c, r, z, nullptr, -1);
        else k::launch_precond(d, c->sym.nRows, c->dDinv.p, r, z, s);
        if (masked) k::launch_mask(n, c->dFixedMask.p, z, s);
    }
    double *col(double *base, int j) const { return base + (size_t)j * (size_t)ld; }
};

// Y (columns colsOut of outBase families) = sum over the input blocks: generic wrapper around launch_block_update.
// C1: rows = all input columns in order, q1 columns (row-major, dense); padded to BLK_MAXC here.
struct UpdCall {
    k::UpdArgs a{};
    std::vector<double> c1, c2;
    int nInTot = 0;
    void inputs(int b, const std::vector<int> &cols) {
        a.nIn[b] = (int)cols.size();
        for (size_t j = 0; j < cols.size(); ++j) a.colIn[b][j] = (unsigned char)cols[j];
    }
    void outputs(int o, const std::vector<int> &cols) {
        a.nOut[o] = (int)cols.size();
        for (size_t j = 0; j < cols.size(); ++j) a.colOut[o][j] = (unsigned char)cols[j];
    }
    void finish() {
        nInTot = a.nIn[0] + a.nIn[1] + a.nIn[2];
        c1.assign((size_t)nInTot * BLK_MAXC, 0.0);
        c2.assign((size_t)nInTot * BLK_MAXC, 0.0);
    }
    // one more family: input blocks in0, in1 (null: none), output block out
    void family(const double *in0, const double *in1, double *out) {
        k::UpdFamily &f = a.fam[a.nFam++];
        f.in[0] = in0; f.in[1] = in1; f.out[0] = out;
    }
    // the three families of the loop's basis [X W P]: the first nIn blocks are the inputs, output o goes to block out0 / out1 (-1: one output)
    void basis(const ModesWork &w, int nIn, int out0, int out1 = -1) {
        for (int f = 0; f < 3; ++f) {
            for (int b = 0; b < nIn; ++b) a.fam[f].in[b] = w.block(f, b);
            a.fam[f].out[0] = w.block(f, out0);
            if (out1 >= 0) a.fam[f].out[1] = w.block(f, out1);
        }
        a.nFam = 3;
    }
};

std::vector<int> iota(int k) {
    std::vector<int> v((size_t)k);
    for (int j = 0; j < k; ++j) v[(size_t)j] = j;
    return v;
}

// the arguments of k_block_residual on the listed columns: R = KX - MX diag(lambda) into w.R (lambda null: zeros)
k::ResArgs res_args(const ModesWork &w, const std::vector<int> &cols, const double *lambda, const double *KX, const double *MX) {
    k::ResArgs ra{};
    ra.n = w.n; ra.ld = w.ld; ra.nc = (int)cols.size(); ra.KX = KX; ra.MX = MX; ra.R = w.R;
    for (size_t j = 0; j < cols.size(); ++j) { ra.col[j] = (unsigned char)cols[j]; ra.lam[j] = lambda ? lambda[j] : 0.0; }
    return ra;
}

void run_update(ModesWork &w, UpdCall &u, bool two) {
    u.a.n = w.n; u.a.ld = w.ld;
    const double *c1 = w.upload_coef(std::move(u.c1));
    const double *c2 = two ? w.upload_coef(std::move(u.c2)) : nullptr;
    k::launch_block_update(u.a, c1, c2, w.s);
}

// M-orthonormalise the columns `cols` of the block V (images MV kept, and KV if non-null) by Cholesky-QR, twice; the Gram matrices come from the
// images. Used for the start block, the rigid modes and the returned columns. false: the Gram matrix is not positive definite.
bool chol_qr_block(ModesWork &w, double *V, double *KV, double *MV, const std::vector<int> &cols) {
    const int k2 = (int)cols.size();
    for (int pass = 0; pass < 2; ++pass) {
        w.lap(-1);
        double *G = w.gram(w.ref(V, cols), w.ref(MV, cols));
        std::vector<double> hG((size_t)k2 * k2), U;
        MFH_HIP(hipMemcpyAsync(hG.data(), G, hG.size() * sizeof(double), hipMemcpyDeviceToHost, w.s));
        w.sync();
        w.lap(3);
        if (chol_qr_factor(k2, hG, 1e-13, U) >= 0) return false;
        UpdCall u;
        u.inputs(0, cols); u.outputs(0, cols);
        u.finish();
        for (int i = 0; i < k2; ++i)
            for (int j = 0; j < k2; ++j) u.c1[(size_t)i * BLK_MAXC + j] = U[(size_t)i * k2 + j];
        u.family(V, nullptr, V);
        u.family(MV, nullptr, MV);
        if (KV) u.family(KV, nullptr, KV);
        run_update(w, u, false);
        w.lap(4);
    }
    return true;
}

// the staging buffers of the block kernels (sizes fixed: a second call keeps them)
void modes_scratch(ModesWork &w) {
    w.gramPart.alloc((size_t)k::GRAM_GRID_CAP * BLK_MAXC * BLK_MAXC);
    w.resPart.alloc((size_t)k::UPD_GRID_CAP * 2 * BLK_MAXC);
    w.small.alloc((size_t)4 * RR_MAX * RR_MAX);
    w.c->stop.alloc(4);                // (control block the preconditioner kernels are handed; no gate here)
    w.c->stop.zero(w.s);
    w.coef.alloc((size_t)8 * RR_MAX * BLK_MAXC);
}

// The known kernel of the free body: translations and infinitesimal rotations about the centre, M-orthonormalised (w.Z, w.MZ; KZ stays zero:
// K Z = 0 up to rounding, and the updates want a K-image of every input block). Once per ModesWork.
void build_rigid_modes(ModesWork &w) {
    if (w.Z) return;
    mfh_ctx *c = w.c;
    hipStream_t s = w.s;
    const size_t L = (size_t)w.ld;
    const HostMesh &hm = c->mesh;
    const int d = w.d, nz = w.nz;
    w.zvec.alloc(L * (size_t)nz * 3);
    w.zvec.zero(s);
    w.Z = w.zvec.p; w.KZ = w.zvec.p + L * nz; w.MZ = w.zvec.p + 2 * L * nz;
    std::vector<double> hz(L * (size_t)nz, 0.0);
    double cen[3] = {0, 0, 0};
    for (int64_t nd = 0; nd < hm.nNode; ++nd)
        for (int a = 0; a < d; ++a) cen[a] += hm.nodePos[(size_t)nd * d + a] / (double)hm.nNode;
    for (int64_t nd = 0; nd < hm.nNode; ++nd) {
        double x[3] = {0, 0, 0};
        for (int a = 0; a < d; ++a) x[a] = hm.nodePos[(size_t)nd * d + a] - cen[a];
        for (int a = 0; a < d; ++a) hz[(size_t)a * L + (size_t)nd * d + a] = 1.0;
        if (d == 3) {
            hz[3 * L + (size_t)nd * 3 + 1] = -x[2]; hz[3 * L + (size_t)nd * 3 + 2] = x[1];
            hz[4 * L + (size_t)nd * 3 + 0] = x[2];  hz[4 * L + (size_t)nd * 3 + 2] = -x[0];
            hz[5 * L + (size_t)nd * 3 + 0] = -x[1]; hz[5 * L + (size_t)nd * 3 + 1] = x[0];
        } else {
            hz[2 * L + (size_t)nd * 2 + 0] = -x[1]; hz[2 * L + (size_t)nd * 2 + 1] = x[0];
        }
    }
    MFH_HIP(hipMemcpyAsync(w.Z, hz.data(), hz.size() * sizeof(double), hipMemcpyHostToDevice, s));
    MFH_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < nz; ++j) w.apply_B(w.col(w.Z, j), w.col(w.MZ, j));
    if (!chol_qr_block(w, w.Z, nullptr, w.MZ, iota(nz))) throw w.fail(MFH_ERR_STATE, "the rigid-body modes of the mesh are linearly dependent");
}

// V -= Z (MZ^T V) on the listed columns of a block (and of its M-image if given); nothing without rigid modes (the clamped case)
void project_out_Z(ModesWork &w, double *V, double *MV, const std::vector<int> &cols) {
    if (!w.Z || cols.empty()) return;
    const int nz = w.nz, k2 = (int)cols.size();
    const std::vector<int> zall = iota(nz);
    w.lap(-1);
    double *G = w.gram(w.ref(w.MZ, zall), w.ref(V, cols));
    std::vector<double> hG((size_t)nz * k2);
    MFH_HIP(hipMemcpyAsync(hG.data(), G, hG.size() * sizeof(double), hipMemcpyDeviceToHost, w.s));
    w.sync();
    w.lap(3);
    UpdCall u;
    u.inputs(0, zall); u.inputs(1, cols); u.outputs(0, cols);
    u.finish();
    for (int i = 0; i < nz; ++i)
        for (int j = 0; j < k2; ++j) u.c1[(size_t)i * BLK_MAXC + j] = -hG[(size_t)i * k2 + j];
    for (int j = 0; j < k2; ++j) u.c1[(size_t)(nz + j) * BLK_MAXC + j] = 1.0;
    u.family(w.Z, V, V);
    if (MV) u.family(w.MZ, MV, MV);
    run_update(w, u, false);
    w.lap(4);
}

// A deflation set on the device (mfh_modes_many): nq B-orthonormal columns Q with their images BQ, both with the blocks' column stride ld
struct DeflationSet {
    const double *Q = nullptr, *BQ = nullptr;
    int nq = 0;
    int nGiven = 0;                    // the leading columns that came from the caller and need not be eigenvectors (see project_residual)
};
void deflate_alloc(ModesWork &w) {
    w.deflPart.alloc((size_t)k::DEFL_GRID_CAP * k::DEFL_MAXQ * BLK_MAXC);
    w.deflG.alloc((size_t)k::DEFL_MAXQ * BLK_MAXC);
    w.deflC.alloc((size_t)k::DEFL_MAXQ * BLK_MAXC);
}
// V -= Q (BQ^T V) on the listed columns of a block (and MV -= BQ (BQ^T V) on its B-image if given): k_deflate_gram, the coefficients through the
// host (the set is B-orthonormal: C = G), k_deflate_update. Returns max |BQ^T V|. One synchronisation.
double deflate_project(ModesWork &w, const DeflationSet &q, double *V, double *MV, const std::vector<int> &cols) {
    if (q.nq == 0 || cols.empty()) return 0.0;
    const int nq = q.nq, k2 = (int)cols.size();
    w.lap(-1);
    const BlockRef r = w.ref(V, cols);
    k::launch_deflate_gram(w.n, q.BQ, w.ld, nq, r, w.deflPart.p, w.deflG.p, w.s);
    std::vector<double> hG((size_t)nq * k2);
    MFH_HIP(hipMemcpyAsync(hG.data(), w.deflG.p, hG.size() * sizeof(double), hipMemcpyDeviceToHost, w.s));
    w.sync();
    double worst = 0.0;
    std::vector<double> hc((size_t)nq * BLK_MAXC, 0.0);
    for (int i = 0; i < nq; ++i)
        for (int j = 0; j < k2; ++j) {
            const double g = hG[(size_t)i * k2 + j];
            hc[(size_t)i * BLK_MAXC + j] = g;
            worst = std::max(worst, std::fabs(g));
        }
    w.staged.push_back(std::move(hc));
    MFH_HIP(hipMemcpyAsync(w.deflC.p, w.staged.back().data(), w.staged.back().size() * sizeof(double), hipMemcpyHostToDevice, w.s));
    k::launch_deflate_update(w.n, q.Q, w.ld, nq, w.deflC.p, r, w.s);
    if (MV) k::launch_deflate_update(w.n, q.BQ, w.ld, nq, w.deflC.p, w.ref(MV, cols), w.s);
    w.lap(7);
    return worst;
}

// The residual of the pencil RESTRICTED to the complement of the caller's columns: an eigenvector x of the restricted pencil has
// A x - lambda B x = B Q mu with multipliers mu, not 0, unless Q spans an invariant subspace. R -= BQ (Q^T R) on the listed columns (the dual of
// deflate_project: R lives in the image space), then the column norms of R once more: k_block_residual with lambda = 0 on R itself leaves R as it
// is (r - 0 mx) and sums r^2. The columns the call itself locked are near-eigenvectors and stay out of this: what they leave in R is the floor
// that mfh_modes_many's final pass measures. norms: the device slot of 2 BLK_MAXC doubles launch_block_residual filled for these columns.
void project_residual(ModesWork &w, const DeflationSet &q, const std::vector<int> &cols, const double *MX, double *norms) {
    if (q.nGiven == 0 || cols.empty()) return;
    const DeflationSet dual{q.BQ, q.Q, q.nGiven, 0};
    deflate_project(w, dual, w.R, nullptr, cols);
    k::launch_block_residual(res_args(w, cols, nullptr, w.R, MX), w.resPart.p, norms, w.s);
}

// ||A x - lambda B x|| / (|lambda| ||B x||) from the squared norms k_block_residual sums
double relative_residual(double r2, double lambda, double mx2) {
    const double den = std::fabs(lambda) * std::sqrt(mx2);
    return den > 0 ? std::sqrt(r2) / den : (r2 == 0.0 ? 0.0 : 1e300);
}

// R = KX - MX diag(lambda) on the columns 0 .. nc - 1 and their relative residuals (out): one download, one synchronisation. given (optional):
// a deflation set whose leading columns came from the caller -- the residuals are then those of the restricted pencil (project_residual: one
// synchronisation more, and the staging slot does not survive it).
void block_residuals(ModesWork &w, const DeflationSet *given, int nc, const double *lambda, const double *KX, const double *MX, double *out) {
    const std::vector<int> cols = iota(nc);
    double *norms = w.small_slot(2 * BLK_MAXC);
    k::launch_block_residual(res_args(w, cols, lambda, KX, MX), w.resPart.p, norms, w.s);
    if (given && given->nGiven > 0) {
        project_residual(w, *given, cols, MX, w.deflG.p);
        norms = w.deflG.p;
    }
    double hn[2 * BLK_MAXC];
    MFH_HIP(hipMemcpyAsync(hn, norms, sizeof(hn), hipMemcpyDeviceToHost, w.s));
    w.sync();
    for (int j = 0; j < nc; ++j) out[j] = relative_residual(hn[2 * j], lambda[j], hn[2 * j + 1]);
}

}   // namespace

extern "C" {

mfh_status mfh_debug_sym_gen_eig(int64_t n, const double *A, const double *B, double *w, double *V) {
    if (n < 1 || n > RR_MAX || !A || !B || !w || !V) return MFH_ERR_INVALID;
    try {
        return sym_gen_eig((int)n, A, B, w, V) ? MFH_OK : MFH_ERR_INVALID;
    } catch (const std::exception &) { return MFH_ERR_INVALID; }
}

mfh_status mfh_debug_block_gram(mfh_ctx *c, int64_t n, int32_t p, int32_t q, const double *A, const double *B, double *G) {
    MFH_TRY(c)
    require(c && A && B && G && n >= 1 && p >= 1 && p <= BLK_MAXC && q >= 1 && q <= BLK_MAXC, MFH_ERR_INVALID, "mfh_debug_block_gram: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t ld = (n + 31) / 32 * 32;
    DBuf<double> a, b, part, g;
    a.alloc((size_t)ld * p); b.alloc((size_t)ld * q); part.alloc((size_t)k::GRAM_GRID_CAP * BLK_MAXC * BLK_MAXC); g.alloc((size_t)p * q);
    MFH_HIP(hipMemcpy2DAsync(a.p, (size_t)ld * sizeof(double), A, (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)p, hipMemcpyHostToDevice, s));
    MFH_HIP(hipMemcpy2DAsync(b.p, (size_t)ld * sizeof(double), B, (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)q, hipMemcpyHostToDevice, s));
    BlockRef ra{}, rb{};
    ra.base = a.p; ra.ld = ld; ra.nc = p;
    rb.base = b.p; rb.ld = ld; rb.nc = q;
    for (int j = 0; j < BLK_MAXC; ++j) ra.col[j] = rb.col[j] = (unsigned char)j;
    k::launch_block_gram(n, ra, rb, part.p, g.p, s);
    g.download(G, (size_t)p * q, s);
    MFH_CATCH(c)
}

mfh_status mfh_time_block_gram(mfh_ctx *c, int64_t n, int32_t p, int32_t q, int32_t reps, double *gram_ms, double *copy_ms) {
    MFH_TRY(c)
    require(c && gram_ms && copy_ms && n >= 1 && reps >= 1 && p >= 1 && p <= BLK_MAXC && q >= 1 && q <= BLK_MAXC, MFH_ERR_INVALID, "mfh_time_block_gram: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t ld = (n + 31) / 32 * 32;
    DBuf<double> ab, dst, part, g;
    ab.alloc((size_t)ld * (p + q)); dst.alloc((size_t)ld * (p + q)); part.alloc((size_t)k::GRAM_GRID_CAP * BLK_MAXC * BLK_MAXC); g.alloc((size_t)p * q);
    k::launch_fill_hash(ld * (p + q), ab.p, s);
    BlockRef ra{}, rb{};
    ra.base = ab.p; ra.ld = ld; ra.nc = p;
    rb.base = ab.p + (size_t)ld * p; rb.ld = ld; rb.nc = q;
    for (int j = 0; j < BLK_MAXC; ++j) ra.col[j] = rb.col[j] = (unsigned char)j;
    for (int r = 0; r < 2; ++r) {      // warm-up of both
        k::launch_block_gram(n, ra, rb, part.p, g.p, s);
        MFH_HIP(hipMemcpyAsync(dst.p, ab.p, (size_t)ld * (p + q) * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    MFH_HIP(hipStreamSynchronize(s));
    {
        EventTimer t(s);
        for (int r = 0; r < reps; ++r) k::launch_block_gram(n, ra, rb, part.p, g.p, s);
        *gram_ms = t.stop() / reps;
    }
    {
        EventTimer t(s);
        for (int r = 0; r < reps; ++r) MFH_HIP(hipMemcpyAsync(dst.p, ab.p, (size_t)ld * (p + q) * sizeof(double), hipMemcpyDeviceToDevice, s));
        *copy_ms = t.stop() / reps;
    }
    MFH_CATCH(c)
}

mfh_status mfh_debug_block_update(mfh_ctx *c, int64_t n, int32_t p, int32_t q, const double *A, const double *C, double *Y) {
    MFH_TRY(c)
    require(c && A && C && Y && n >= 1 && p >= 1 && p <= BLK_MAXC && q >= 1 && q <= BLK_MAXC, MFH_ERR_INVALID, "mfh_debug_block_update: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t ld = (n + 31) / 32 * 32;
    DBuf<double> a, y, coef;
    a.alloc((size_t)ld * p); y.alloc((size_t)ld * q);
    MFH_HIP(hipMemcpy2DAsync(a.p, (size_t)ld * sizeof(double), A, (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)p, hipMemcpyHostToDevice, s));
    std::vector<double> hc((size_t)p * BLK_MAXC, 0.0);
    for (int i = 0; i < p; ++i)
        for (int j = 0; j < q; ++j) hc[(size_t)i * BLK_MAXC + j] = C[(size_t)i * q + j];
    coef.upload(hc, s);
    k::UpdArgs u{};
    u.n = n; u.ld = ld; u.nIn[0] = p; u.nOut[0] = q; u.nFam = 1;
    for (int j = 0; j < BLK_MAXC; ++j) u.colIn[0][j] = u.colOut[0][j] = (unsigned char)j;
    u.fam[0].in[0] = a.p; u.fam[0].out[0] = y.p;
    k::launch_block_update(u, coef.p, nullptr, s);
    MFH_HIP(hipMemcpy2DAsync(Y, (size_t)n * sizeof(double), y.p, (size_t)ld * sizeof(double), (size_t)n * sizeof(double), (size_t)q, hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

mfh_status mfh_debug_deflate(mfh_ctx *c, int64_t n, int32_t nq, int32_t nv, int32_t k2, const int32_t *cols, const double *BQ, const double *Q, const double *V,
                             double *G, double *Vout) {
    MFH_TRY(c)
    require(c && cols && BQ && Q && V && G && Vout && n >= 1 && nq >= 1 && nq <= k::DEFL_MAXQ && nv >= 1 && nv <= BLK_MAXC && k2 >= 1 && k2 <= nv, MFH_ERR_INVALID,
            "mfh_debug_deflate: arguments");
    for (int j = 0; j < k2; ++j) {
        require(cols[j] >= 0 && cols[j] < nv, MFH_ERR_INVALID, "mfh_debug_deflate: column out of range");
        for (int i = 0; i < j; ++i) require(cols[i] != cols[j], MFH_ERR_INVALID, "mfh_debug_deflate: column listed twice");
    }
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t ld = (n + 31) / 32 * 32;
    DBuf<double> bq, q, v, part, g, coef;
    bq.alloc((size_t)ld * nq); q.alloc((size_t)ld * nq); v.alloc((size_t)ld * nv);
    part.alloc((size_t)k::DEFL_GRID_CAP * k::DEFL_MAXQ * BLK_MAXC); g.alloc((size_t)nq * k2);
    const size_t rowBytes = (size_t)n * sizeof(double), ldBytes = (size_t)ld * sizeof(double);
    MFH_HIP(hipMemcpy2DAsync(bq.p, ldBytes, BQ, rowBytes, rowBytes, (size_t)nq, hipMemcpyHostToDevice, s));
    MFH_HIP(hipMemcpy2DAsync(q.p, ldBytes, Q, rowBytes, rowBytes, (size_t)nq, hipMemcpyHostToDevice, s));
    MFH_HIP(hipMemcpy2DAsync(v.p, ldBytes, V, rowBytes, rowBytes, (size_t)nv, hipMemcpyHostToDevice, s));
    BlockRef rv{};
    rv.base = v.p; rv.ld = ld; rv.nc = k2;
    for (int j = 0; j < k2; ++j) rv.col[j] = (unsigned char)cols[j];
    k::launch_deflate_gram(n, bq.p, ld, nq, rv, part.p, g.p, s);
    g.download(G, (size_t)nq * k2, s);
    std::vector<double> hc((size_t)nq * BLK_MAXC, 0.0);
    for (int i = 0; i < nq; ++i)
        for (int j = 0; j < k2; ++j) hc[(size_t)i * BLK_MAXC + j] = G[(size_t)i * k2 + j];
    coef.upload(hc, s);
    k::launch_deflate_update(n, q.p, ld, nq, coef.p, rv, s);
    MFH_HIP(hipMemcpy2DAsync(Vout, rowBytes, v.p, ldBytes, rowBytes, (size_t)nv, hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

mfh_status mfh_time_deflate(mfh_ctx *c, int64_t n, int32_t nq, int32_t k2, int32_t reps, double *gram_ms, double *update_ms, double *copy_ms) {
    MFH_TRY(c)
    require(c && gram_ms && update_ms && copy_ms && n >= 1 && reps >= 1 && nq >= 1 && nq <= k::DEFL_MAXQ && k2 >= 1 && k2 <= BLK_MAXC, MFH_ERR_INVALID,
            "mfh_time_deflate: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t ld = (n + 31) / 32 * 32;
    const size_t count = (size_t)ld * (size_t)(nq + k2);
    DBuf<double> qv, dst, part, g, coef;
    qv.alloc(count); dst.alloc(count); part.alloc((size_t)k::DEFL_GRID_CAP * k::DEFL_MAXQ * BLK_MAXC); g.alloc((size_t)nq * k2);
    k::launch_fill_hash((int64_t)count, qv.p, s);
    std::vector<double> hc((size_t)nq * BLK_MAXC, 0.0);          // zero coefficients: the update leaves V as it is, repeat after repeat
    coef.upload(hc, s);
    BlockRef rv{};
    rv.base = qv.p + (size_t)ld * nq; rv.ld = ld; rv.nc = k2;
    for (int j = 0; j < BLK_MAXC; ++j) rv.col[j] = (unsigned char)j;
    for (int r = 0; r < 2; ++r) {      // warm-up of all three
        k::launch_deflate_gram(n, qv.p, ld, nq, rv, part.p, g.p, s);
        k::launch_deflate_update(n, qv.p, ld, nq, coef.p, rv, s);
        MFH_HIP(hipMemcpyAsync(dst.p, qv.p, count * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    MFH_HIP(hipStreamSynchronize(s));
    {
        EventTimer t(s);
        for (int r = 0; r < reps; ++r) k::launch_deflate_gram(n, qv.p, ld, nq, rv, part.p, g.p, s);
        *gram_ms = t.stop() / reps;
    }
    {
        EventTimer t(s);
        for (int r = 0; r < reps; ++r) k::launch_deflate_update(n, qv.p, ld, nq, coef.p, rv, s);
        *update_ms = t.stop() / reps;
    }
    {
        EventTimer t(s);
        for (int r = 0; r < reps; ++r) MFH_HIP(hipMemcpyAsync(dst.p, qv.p, count * sizeof(double), hipMemcpyDeviceToDevice, s));
        *copy_ms = t.stop() / reps;
    }
    MFH_CATCH(c)
}

}   // extern "C"

namespace {

// What mfh_debug_lobpcg sees of a run: per call of converged() the m Ritz values, the m relative residuals and {|wact|, |pact|, restarts so far} (the
// sets are those the iteration before used), and the whole block X as the loop left it, before return_columns touches it
struct LoopTrace {
    std::vector<double> lam, res;
    std::vector<int32_t> sets;
    double *X = nullptr;               // host, m x n
};
// What a run of the loop is given, beside the ModesWork its caller prepared
struct LoopIn {
    int nev;
    bool freeBody;
    double rtol;
    int maxit;
    double *lambda, *X, *residuals;    // the outputs on the host: nev eigenvalues, nev x n modes, nev relative residuals (optional)
    const double *X0 = nullptr;        // a warm start (host, nX0 x n): its rows take the place of the first nX0 columns of the start block as they are, masked
    int nX0 = -1;                      // ... its column count (-1: nev; the test hook mfh_debug_lobpcg gives the whole block, m)
    const DeflationSet *defl = nullptr;
    const double *X0dev = nullptr;     // ... or nX0dev columns from the device (stride ld, already in the space: the guard columns of an earlier batch)
    int nX0dev = 0;
    LoopTrace *trace = nullptr;        // the history of the run (mfh_debug_lobpcg; null for every entry point: nothing is recorded, nothing launched)
};
struct LoopOut {
    std::vector<double> sign;          // per returned column: -1 where the sign rule flipped the host copy (the device column keeps its sign)
    int iterations = 0, restarts = 0, locked = 0, blockSize = 0;
    bool done = false;
    double maxResidual = 0, setupMs = 0, solveMs = 0;
    double lockDefect = 0;             // with a deflation set: max |BQ^T X| of the returned columns before their last projection
};

// The state of one run of the loop and its steps. The basis of an iteration is S = [X W P]: all m columns of X, the columns wact of W (the
// preconditioned residuals of the columns that have not converged) and the columns pact of P (the previous directions).
struct Lobpcg {
    ModesWork &w;
    const LoopIn &in;
    const int nq;                      // columns of the deflation set
    int m = 0;                         // block size
    std::vector<int> all, wact, pact;
    std::vector<double> lam, res;
    std::vector<uint8_t> conv;
    bool haveP = false;
    int restarts = 0;

    static int block_size(int nev, int64_t nEff) { return (int)std::min<int64_t>(std::min(nev + std::max(2, (nev + 3) / 4), BLK_MAXC), nEff); }

    // block size, the ten blocks, the staging buffers
    Lobpcg(ModesWork &w_, const LoopIn &in_) : w(w_), in(in_), nq(in_.defl ? in_.defl->nq : 0) {
        w.nz = in.freeBody ? (w.d == 3 ? 6 : 3) : 0;
        const int64_t nEff = w.n - (int64_t)w.c->fixedVars.size() - w.nz - nq;   // dimension of the space the iteration lives in
        w.need(in.nev <= nEff, MFH_ERR_INVALID, "more modes asked for than the pencil has");
        m = block_size(in.nev, nEff);
        w.m = m;
        const size_t L = (size_t)w.ld;
        w.vec.alloc(L * (size_t)m * 10);
        w.vec.zero(w.s);
        double *b0 = w.vec.p;
        w.X = b0; w.W = b0 + L * m; w.P = b0 + 2 * L * m; w.KX = b0 + 3 * L * m; w.KW = b0 + 4 * L * m; w.KP = b0 + 5 * L * m;
        w.MX = b0 + 6 * L * m; w.MW = b0 + 7 * L * m; w.MP = b0 + 8 * L * m; w.R = b0 + 9 * L * m;
        modes_scratch(w);
        all = iota(m);
        lam.assign((size_t)m, 0.0);
        res.assign((size_t)m, 0.0);
        conv.assign((size_t)m, 0);
    }

    // start block: hashed values, smoothed once by the preconditioner (or the caller's / the earlier batch's columns), in the complement of Z and
    // of the deflation set, M-orthonormal; then Rayleigh-Ritz on it (the generalised problem: X^T K X against X^T M X)
    void start_block() {
        mfh_ctx *c = w.c;
        hipStream_t s = w.s;
        k::launch_fill_hash((int64_t)w.ld * m, w.W, s);
        for (int j = 0; j < m; ++j) {
            if (w.masked) k::launch_mask(w.n, c->dFixedMask.p, w.col(w.W, j), s);
            w.precond(w.col(w.W, j), w.col(w.X, j));
        }
        if (in.X0) {
            const int nx0 = in.nX0 < 0 ? in.nev : in.nX0;
            w.need(nx0 >= 1 && nx0 <= m, MFH_ERR_INVALID, "the warm start has more columns than the block");
            MFH_HIP(hipMemcpy2DAsync(w.X, (size_t)w.ld * sizeof(double), in.X0, (size_t)w.n * sizeof(double), (size_t)w.n * sizeof(double), (size_t)nx0, hipMemcpyHostToDevice, s));
            if (w.masked)
                for (int j = 0; j < nx0; ++j) k::launch_mask(w.n, c->dFixedMask.p, w.col(w.X, j), s);
            MFH_HIP(hipStreamSynchronize(s));
        }
        if (in.X0dev && in.nX0dev > 0)
            MFH_HIP(hipMemcpyAsync(w.X, in.X0dev, (size_t)w.ld * std::min(in.nX0dev, m) * sizeof(double), hipMemcpyDeviceToDevice, s));
        project_out_Z(w, w.X, nullptr, all);
        if (nq > 0)
            for (int pass = 0; pass < 2; ++pass) deflate_project(w, *in.defl, w.X, nullptr, all);
        for (int j = 0; j < m; ++j) w.apply_B(w.col(w.X, j), w.col(w.MX, j));
        if (!chol_qr_block(w, w.X, nullptr, w.MX, all)) throw w.fail(MFH_ERR_STATE, "the start block is rank deficient");
        w.apply_images(w.X, w.KX, w.MX, all, false);
        double *GK = w.gram(w.ref(w.X, all), w.ref(w.KX, all));
        double *GM = w.gram(w.ref(w.X, all), w.ref(w.MX, all));
        std::vector<double> hK((size_t)m * m), hM((size_t)m * m), V((size_t)m * m);
        MFH_HIP(hipMemcpyAsync(hK.data(), GK, hK.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        MFH_HIP(hipMemcpyAsync(hM.data(), GM, hM.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        w.sync();
        if (!sym_gen_eig(m, hK.data(), hM.data(), lam.data(), V.data())) throw w.fail(MFH_ERR_STATE, "the start block lost its M-orthonormality");
        UpdCall u;
        u.inputs(0, all); u.outputs(0, all);
        u.finish();
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) u.c1[(size_t)i * BLK_MAXC + j] = V[(size_t)i * m + j];
        u.basis(w, 1, 0);
        run_update(w, u, false);
    }

    // residuals of all columns (R, ||R||, ||MX||): one download. true: the first nev columns have converged.
    bool converged() {
        block_residuals(w, in.defl, m, lam.data(), w.KX, w.MX, res.data());
        w.lap(5);
        for (int j = 0; j < m; ++j) {
            if (!std::isfinite(res[(size_t)j])) throw w.fail(MFH_ERR_NOT_CONVERGED, "breakdown (a residual is not finite)");
            conv[(size_t)j] = res[(size_t)j] <= in.rtol;
        }
        bool done = true;
        for (int j = 0; j < in.nev; ++j) done = done && conv[(size_t)j];
        return done;
    }

    // (mfh_debug_lobpcg) what the call of converged() just made, and the sets of the iteration before it
    void record(LoopTrace &t) const {
        t.lam.insert(t.lam.end(), lam.begin(), lam.end());
        t.res.insert(t.res.end(), res.begin(), res.end());
        t.sets.push_back((int32_t)wact.size()); t.sets.push_back((int32_t)pact.size()); t.sets.push_back((int32_t)restarts);
    }
    void record_block(LoopTrace &t) const {
        if (!t.X) return;
        MFH_HIP(hipMemcpy2DAsync(t.X, (size_t)w.n * sizeof(double), w.X, (size_t)w.ld * sizeof(double), (size_t)w.n * sizeof(double), (size_t)m, hipMemcpyDeviceToHost, w.s));
        MFH_HIP(hipStreamSynchronize(w.s));
    }

    // W = the preconditioned residuals of the active columns, in the complement of Z and of the deflation set, with their images. Soft locking:
    // converged columns stay in X, their W and P columns leave the basis.
    void new_directions() {
        std::vector<int> act;
        for (int j = 0; j < m; ++j)
            if (!conv[(size_t)j]) act.push_back(j);
        for (int j : act) w.precond(w.col(w.R, j), w.col(w.W, j));
        w.lap(2);
        project_out_Z(w, w.W, nullptr, act);
        if (nq > 0) deflate_project(w, *in.defl, w.W, nullptr, act);
        w.apply_images(w.W, w.KW, w.MW, act, true);
        pact = haveP ? act : std::vector<int>();
        wact = std::move(act);
    }

    // host Gram matrix S^T (img S) of the basis, kb x kb row-major, against its A-images (img 1) or B-images (img 2): the block Grams of the upper
    // block triangle, downloaded and mirrored. One synchronisation.
    std::vector<double> basis_gram(int img) {
        const std::vector<int> *cl[3] = {&all, &wact, &pact};
        const int kb = m + (int)wact.size() + (int)pact.size();
        const int off[3] = {0, m, m + (int)wact.size()};
        struct Part { int bi, bj; double *dev; std::vector<double> host; };
        std::vector<Part> parts;
        parts.reserve(6);              // (asynchronous downloads point into the elements: no reallocation)
        for (int bi = 0; bi < 3; ++bi)
            for (int bj = bi; bj < 3; ++bj)
                if (!cl[bi]->empty() && !cl[bj]->empty())
                    parts.push_back(Part{bi, bj, w.gram(w.ref(w.block(0, bi), *cl[bi]), w.ref(w.block(img, bj), *cl[bj])), std::vector<double>(cl[bi]->size() * cl[bj]->size())});
        for (Part &p : parts) MFH_HIP(hipMemcpyAsync(p.host.data(), p.dev, p.host.size() * sizeof(double), hipMemcpyDeviceToHost, w.s));
        w.sync();
        w.lap(3);
        std::vector<double> G((size_t)kb * kb, 0.0);
        for (const Part &p : parts) {
            const int ni = (int)cl[p.bi]->size(), nj = (int)cl[p.bj]->size();
            for (int i = 0; i < ni; ++i)
                for (int j = 0; j < nj; ++j) {
                    G[(size_t)(off[p.bi] + i) * kb + off[p.bj] + j] = p.host[(size_t)i * nj + j];
                    if (p.bi != p.bj) G[(size_t)(off[p.bj] + j) * kb + off[p.bi] + i] = p.host[(size_t)i * nj + j];
                }
        }
        return G;
    }

    // Cholesky-QR of the basis, twice: Gram-Schmidt in the order X, W, P, so W leaves M-orthogonal to X. A pivot that fails in P restarts (P leaves
    // the basis for this iteration); one that fails in W drops that column of W, and P with it; one in X is a breakdown.
    void orthonormalise() {
        for (int pass = 0; pass < 2; ++pass)
            for (int attempt = 0;; ++attempt) {
                w.need(attempt < 2 * BLK_MAXC + 2, MFH_ERR_NOT_CONVERGED, "breakdown (the basis cannot be orthonormalised)");
                const int nw = (int)wact.size(), np = (int)pact.size(), kb = m + nw + np;
                const std::vector<double> G = basis_gram(2);
                std::vector<double> U;
                const int bad = chol_qr_factor(kb, G, 1e-12, U);
                if (bad >= m + nw) { pact.clear(); haveP = false; ++restarts; continue; }
                if (bad >= m) { wact.erase(wact.begin() + (bad - m)); if (!pact.empty()) { pact.clear(); haveP = false; ++restarts; } continue; }
                if (bad >= 0) throw w.fail(MFH_ERR_NOT_CONVERGED, "breakdown (the Ritz block lost its rank)");
                // S <- S U, images alike: first W and P (they read the old X), then X
                if (nw + np > 0) {
                    UpdCall u;
                    u.inputs(0, all); u.inputs(1, wact); u.inputs(2, pact);
                    u.outputs(0, wact); u.outputs(1, pact);
                    u.finish();
                    for (int i = 0; i < kb; ++i) {
                        for (int j = 0; j < nw; ++j) u.c1[(size_t)i * BLK_MAXC + j] = U[(size_t)i * kb + m + j];
                        for (int j = 0; j < np; ++j) u.c2[(size_t)i * BLK_MAXC + j] = U[(size_t)i * kb + m + nw + j];
                    }
                    u.a.skip2 = 0;
                    u.basis(w, 3, 1, 2);
                    run_update(w, u, np > 0);
                }
                UpdCall u;
                u.inputs(0, all); u.outputs(0, all);
                u.finish();
                for (int i = 0; i < m; ++i)
                    for (int j = 0; j < m; ++j) u.c1[(size_t)i * BLK_MAXC + j] = U[(size_t)i * kb + j];
                u.basis(w, 1, 0);
                run_update(w, u, false);
                w.lap(4);
                break;
            }
    }

    // Rayleigh-Ritz on the M-orthonormal basis (S^T K S, a standard problem): X+ = S C, P+ = [W P] C' (C' = the W and P rows of C), and the same
    // combinations of the K- and M-images
    void rayleigh_ritz() {
        const int nw = (int)wact.size(), kb = m + nw + (int)pact.size();
        std::vector<double> G = basis_gram(1);
        for (int i = 0; i < kb; ++i)
            for (int j = i + 1; j < kb; ++j) G[(size_t)i * kb + j] = G[(size_t)j * kb + i] = 0.5 * (G[(size_t)i * kb + j] + G[(size_t)j * kb + i]);
        std::vector<double> ev((size_t)kb), V((size_t)kb * kb);
        sym_gen_eig(kb, G.data(), nullptr, ev.data(), V.data());
        w.lap(6);
        UpdCall u;
        u.inputs(0, all); u.inputs(1, wact); u.inputs(2, pact);
        u.outputs(0, all); u.outputs(1, all);
        u.finish();
        for (int i = 0; i < kb; ++i)
            for (int j = 0; j < m; ++j) {
                u.c1[(size_t)i * BLK_MAXC + j] = V[(size_t)i * kb + j];
                if (i >= m) u.c2[(size_t)i * BLK_MAXC + j] = V[(size_t)i * kb + j];
            }
        u.a.skip2 = m;
        u.basis(w, 3, 0, 2);
        run_update(w, u, true);
        w.lap(4);
        for (int j = 0; j < m; ++j) lam[(size_t)j] = ev[(size_t)j];
        haveP = nw > 0;
    }

    // the returned columns: in the complement of the deflation set once more, one final M-orthonormalisation, download (where the solve timer
    // stops); on the host the sign rule and exact zeros on the fixed variables
    void return_columns(EventTimer &tsolve, LoopOut &o) {
        const std::vector<int> ret = iota(in.nev);
        if (w.recompute_returned_B())
            for (int j : ret) w.apply_B(w.col(w.X, j), w.col(w.MX, j));
        if (nq > 0) o.lockDefect = deflate_project(w, *in.defl, w.X, w.MX, ret);
        if (!chol_qr_block(w, w.X, nullptr, w.MX, ret)) throw w.fail(MFH_ERR_NOT_CONVERGED, "breakdown (the returned modes lost their rank)");
        MFH_HIP(hipMemcpy2DAsync(in.X, (size_t)w.n * sizeof(double), w.X, (size_t)w.ld * sizeof(double), (size_t)w.n * sizeof(double), (size_t)in.nev, hipMemcpyDeviceToHost, w.s));
        MFH_HIP(hipStreamSynchronize(w.s));
        o.solveMs = tsolve.stop();
        o.sign.assign((size_t)in.nev, 1.0);
        for (int j = 0; j < in.nev; ++j) {
            double *x = in.X + (size_t)j * (size_t)w.n;
            int64_t at = 0;
            for (int64_t i = 1; i < w.n; ++i)
                if (std::fabs(x[i]) > std::fabs(x[at])) at = i;
            if (x[at] < 0) {
                o.sign[(size_t)j] = -1.0;
                for (int64_t i = 0; i < w.n; ++i) x[i] = -x[i];
            }
            if (w.masked)
                for (int64_t fv : w.c->fixedVars) x[(size_t)fv] = 0.0;       // (exactly +0.0: the iteration keeps them at +-0.0)
            in.lambda[j] = lam[(size_t)j];
            if (in.residuals) in.residuals[j] = res[(size_t)j];
        }
    }
};

// The block LOBPCG loop on the pencil (A, B) of w (the product members of ModesWork): the nev smallest eigenpairs of A x = lambda B x, B-orthonormal
// columns with the sign rule, the relative residuals ||A x - lambda B x|| / (|lambda| ||B x||). The caller has prepared the context and w
// (modes_prepare); tsetup is its running set-up timer. Shared by mfh_modes, mfh_modes_many, mfh_buckling and mfh_modes_prestressed.
// in.defl (optional): a deflation set. The loop then runs in the B-orthogonal complement of its columns (and of Z): the start block is projected
// twice and every preconditioned residual block once, nEff loses nq, and before the final orthonormalisation the returned columns and their
// B-images are projected once more (o.lockDefect = the largest |BQ^T X| seen there). Without a set, a warm start or a device seed the operations
// are those of the loop without them.
void lobpcg_run(ModesWork &w, const LoopIn &in, EventTimer &tsetup, LoopOut &o) {
    Lobpcg L(w, in);
    if (in.freeBody) build_rigid_modes(w);         // the known kernel of the free body
    L.start_block();
    MFH_HIP(hipStreamSynchronize(w.s));
    o.setupMs = tsetup.stop();
    EventTimer tsolve(w.s);
    w.lap(-1);
    int it = 0;
    for (;; ++it) {
        o.done = L.converged();
        if (in.trace) L.record(*in.trace);
        if (o.done || it >= in.maxit) break;
        L.new_directions();
        L.orthonormalise();
        L.rayleigh_ritz();
    }
    if (in.trace) L.record_block(*in.trace);
    L.return_columns(tsolve, o);
    if (w.timing)
        fprintf(stderr, "[%s] n %lld m %d iterations %d | ms: K %.3f M %.3f precond %.3f gram %.3f update %.3f residual %.3f rayleigh-ritz(host+sync) %.3f deflation %.3f\n",
                w.who, (long long)w.n, L.m, it, w.tPhase[0], w.tPhase[1], w.tPhase[2], w.tPhase[3], w.tPhase[4], w.tPhase[5], w.tPhase[6], w.tPhase[7]);
    o.iterations = it; o.restarts = L.restarts; o.blockSize = L.m;
    for (int j = 0; j < L.m; ++j) o.locked += L.conv[(size_t)j] ? 1 : 0;
    for (int j = 0; j < in.nev; ++j) o.maxResidual = std::max(o.maxResidual, L.res[(size_t)j]);
}

// ---- what the four entry points share: the state they hold for the duration of the call, the contexts they accept, the set-up, the finish
void modes_note(mfh_ctx *c, const std::string &t) {
    if (!c->modesNote.empty()) c->modesNote += "; ";
    c->modesNote += t;
}
// WideGuard (both triangles of the pattern for the duration of the call, in force before ensure_precond runs) with the call's note started and,
// at the end, the solver's singular-system switch restored. Before the set-up timer starts.
struct ModesGuard : WideGuard {
    explicit ModesGuard(mfh_ctx *c_) : WideGuard(c_) {
        c->modesNote.clear();
        if (widened) modes_note(c, "the pattern held the upper triangle only: symbolic phase re-run with both triangles (what option matrix_storage 0 does) for this call");
    }
    ~ModesGuard() { c->tlSuppress = false; }
};
// the refusals of mfh_modes and mfh_modes_many that need no device work (after require_device)
void modes_require_context(mfh_ctx *c, bool freeBody, const std::string &who) {
    if (!(c->op == MFH_OP_ELASTICITY && c->opDegree != 1))
        throw Error(MFH_ERR_UNSUPPORTED, who + ": the pencil is (elasticity, mass) on the mesh's own degree: select MFH_OP_ELASTICITY and leave the forced-degree-1 view");
    if (!(!dist_active(c) && c->mesh.nOwned == c->mesh.nNode && c->nOwnedDoF() == c->nDoF)) throw Error(MFH_ERR_UNSUPPORTED, who + ": unpartitioned contexts only");
    if (!(c->mesh.dim == 2 || c->mesh.dim == 3)) throw Error(MFH_ERR_UNSUPPORTED, who + ": 2D / 3D meshes");
    if (freeBody) {
        if (!(c->fixedVars.empty() && c->dofForNode.empty())) throw Error(MFH_ERR_UNSUPPORTED, who + ": the free-free case takes no fixed variables and the identity DoF map");
    } else {
        const int q = free_rigid_motions(c);
        if (q > 0) throw Error(MFH_ERR_UNSUPPORTED, "the fixed variables leave " + std::to_string(q) + " rigid motions free: the clamped pencil is singular (fix more variables, or ask for MFH_MODES_FREE)");
    }
}
struct ModesSetup {
    const char *who;                   // the entry point, for messages
    Pencil pencil;
    bool freeBody;
    double density, loadFactor;
    bool mass, geometric;              // the one-double-per-block buffers the pencil's products read (assembled in this order; none is started that is not asked for)
};
// The preconditioner of K (what the next solve of this kind would use; it plays the part of the inverse in every pencil), the pencil's buffers
// and the fields of w up to useTL. Under a ModesGuard.
void modes_prepare(mfh_ctx *c, const ModesSetup &su, ModesWork &w) {
    const std::string who = su.who;
    c->tlSuppress = su.freeBody;
    ensure_precond(c);
    if (su.freeBody) {
        c->precondNote.clear();
        if (c->precond == MFH_PRECOND_MULTIGRID && ensure_multigrid(c)) modes_note(c, "multigrid preconditioner on the singular K of the free body: dense level pinned");
        else if (c->precond == MFH_PRECOND_TWO_LEVEL || c->precond == MFH_PRECOND_MULTIGRID) modes_note(c, "two-level / multigrid preconditioner unavailable on the singular K of the free body: using block-Jacobi");
    } else
        ensure_coarse_levels(c, 1);
    if (c->sym.nRows != c->sym.nCols) throw Error(MFH_ERR_UNSUPPORTED, who + ": unpartitioned contexts only");
    if (su.mass) ensure_mass(c);
    if (su.geometric) ensure_geometric(c);
    prepare_matrix_free(c);
    if (!c->use_mf()) require_full_storage(c, ("the assembled SpMV of " + who).c_str());

    w.c = c; w.s = c->stream; w.d = c->bs();
    w.n = (int64_t)w.d * c->nDoF; w.ld = (w.n + 31) / 32 * 32;
    w.pencil = su.pencil;
    w.density = su.density;
    w.loadFactor = su.loadFactor;
    w.who = su.who;
    w.masked = !c->fixedVars.empty();
    w.timing = getenv("MFH_MODES_TIMING") != nullptr;
    w.useMG = c->precond == MFH_PRECOND_MULTIGRID && c->mg.valid && c->mg.singular == c->tlSuppress;
    w.useTL = !w.useMG && (c->precond == MFH_PRECOND_TWO_LEVEL || c->precond == MFH_PRECOND_MULTIGRID) && c->tl.valid && !c->tlSuppress;
    if (!su.freeBody && !w.useMG && !w.useTL && (c->precond == MFH_PRECOND_TWO_LEVEL || c->precond == MFH_PRECOND_MULTIGRID) && !c->precondNote.empty()) modes_note(c, c->precondNote);
}
int modes_precond_used(const mfh_ctx *c, const ModesWork &w) {
    return w.useMG ? MFH_PRECOND_MULTIGRID : (w.useTL ? MFH_PRECOND_TWO_LEVEL : ((c->precond == MFH_PRECOND_TWO_LEVEL || c->precond == MFH_PRECOND_MULTIGRID) ? (int)MFH_PRECOND_BLOCK_JACOBI : c->precond));
}
// the fields mfh_modes_info and mfh_buckling_info share
template <class Info>
void modes_fill_info(Info *info, const mfh_ctx *c, const ModesWork &w, const LoopOut &lo) {
    if (!info) return;
    info->converged = lo.done ? 1 : 0;
    info->iterations = lo.iterations;
    info->nLocked = lo.locked;
    info->precondUsed = modes_precond_used(c, w);
    info->blockSize = lo.blockSize;
    info->restarts = lo.restarts;
    info->maxResidual = lo.maxResidual;
    info->solve_ms = lo.solveMs;
    info->setup_ms = lo.setupMs;
    info->note = c->modesNote.c_str();
}
void require_converged(const LoopOut &lo) {
    if (!lo.done) throw Error(MFH_ERR_NOT_CONVERGED, "LOBPCG did not reach the requested tolerance within maxit iterations");
}

// ---- the steps of mfh_modes_many. Its deflation set is Q and M Q (device, stride ld), resident for the call: the caller's nLocked columns, then what the batches found.
// M-orthonormalise the caller's Q (masked, and in the free case in the complement of Z): block Gram-Schmidt over groups of <= 24 columns -- a group
// is projected twice against the groups before it (k_deflate_gram / k_deflate_update), then Cholesky-QR'd on the host
void many_orthonormalise_given(ModesWork &w, bool freeBody, const double *Qin, int nLocked, double *Q, double *BQ) {
    hipStream_t s = w.s;
    const char *deficient = "Q is rank deficient (its Gram matrix Q^T M Q is not positive definite)";
    MFH_HIP(hipMemcpy2DAsync(Q, (size_t)w.ld * sizeof(double), Qin, (size_t)w.n * sizeof(double), (size_t)w.n * sizeof(double), (size_t)nLocked, hipMemcpyHostToDevice, s));
    if (w.masked)
        for (int j = 0; j < nLocked; ++j) k::launch_mask(w.n, w.c->dFixedMask.p, w.col(Q, j), s);
    MFH_HIP(hipStreamSynchronize(s));
    if (freeBody) build_rigid_modes(w);
    for (int g0 = 0; g0 < nLocked; g0 += BLK_MAXC) {
        const int kg = std::min(BLK_MAXC, nLocked - g0);
        const std::vector<int> cols = iota(kg);
        double *Vg = w.col(Q, g0), *MVg = w.col(BQ, g0);
        if (freeBody) project_out_Z(w, Vg, nullptr, cols);
        for (int j = 0; j < kg; ++j) w.apply_B(w.col(Vg, j), w.col(MVg, j));
        auto norms2 = [&]() {
            double *G = w.gram(w.ref(Vg, cols), w.ref(MVg, cols));
            std::vector<double> hG((size_t)kg * kg), dd((size_t)kg);
            MFH_HIP(hipMemcpyAsync(hG.data(), G, hG.size() * sizeof(double), hipMemcpyDeviceToHost, s));
            w.sync();
            for (int j = 0; j < kg; ++j) dd[(size_t)j] = hG[(size_t)j * kg + j];
            return dd;
        };
        const std::vector<double> d0 = norms2();
        if (g0 > 0) {
            const DeflationSet prev{Q, BQ, g0, 0};
            for (int pass = 0; pass < 2; ++pass) deflate_project(w, prev, Vg, MVg, cols);
            const std::vector<double> d1 = norms2();
            for (int j = 0; j < kg; ++j)
                if (!(d1[(size_t)j] > 1e-13 * d0[(size_t)j])) throw w.fail(MFH_ERR_INVALID, deficient);
        }
        for (int j = 0; j < kg; ++j)
            if (!(d0[(size_t)j] > 0.0)) throw w.fail(MFH_ERR_INVALID, deficient);
        if (!chol_qr_block(w, Vg, nullptr, MVg, cols)) throw w.fail(MFH_ERR_INVALID, deficient);
    }
    for (int j = 0; j < nLocked; ++j) w.apply_B(w.col(Q, j), w.col(BQ, j));      // the images afresh: they went through every update
}

struct ManyRun {
    int found = 0, batches = 0, iterations = 0, restarts = 0;
    bool allDone = true, exhausted = false;
    double setupMs = 0, solveMs = 0, lockDefect = 0;
    std::vector<double> res;           // per mode found, in the order found
    std::vector<int> batchOf;
    std::vector<double> sign;          // of every found column, in the order found (LoopOut::sign)
};
// Batch by batch: each runs the loop in the complement of the set (to rtol lockFactor, the last one of a sweep without a band to rtol), joins the
// set with fresh images, and its guard columns seed the next start block. Ends at nev modes, at a batch that did not converge, or past the band.
void many_batches(ModesWork &w, const mfh_modes_many_params &p, int batch, double lockFactor, bool band, EventTimer &tsetup, double *Q, double *BQ,
                  double *lambda, double *Xout, ManyRun &r) {
    hipStream_t s = w.s;
    const size_t L = (size_t)w.ld;
    const int nev = p.nev;
    const bool useSeed = getenv("MFH_MODES_MANY_NO_SEED") == nullptr;      // (scripts/probe_many_modes.py measures what the seeding saves)
    DBuf<double> seed;
    int nqNow = p.nLocked, nSeed = 0;
    r.res.assign((size_t)nev, 0.0);
    r.batchOf.assign((size_t)nev, 0);
    while (r.found < nev) {
        const int nb = std::min(batch, nev - r.found);
        const bool last = !band && r.found + nb == nev;
        const DeflationSet ds{Q, BQ, nqNow, p.nLocked};
        LoopIn in{nb, (p.flags & MFH_MODES_FREE) != 0, last ? p.rtol : p.rtol * lockFactor, p.maxit, lambda + r.found, Xout + (size_t)r.found * (size_t)w.n, r.res.data() + r.found};
        LoopOut lo;
        if (r.batches == 0) {
            if (nqNow) in.defl = &ds;
            lobpcg_run(w, in, tsetup, lo);
        } else {
            in.defl = &ds;
            in.X0dev = nSeed > 0 ? seed.p : nullptr;
            in.nX0dev = nSeed;
            EventTimer tb(s);
            lobpcg_run(w, in, tb, lo);
        }
        if (w.timing || getenv("MFH_MODES_MANY_LOG")) fprintf(stderr, "[mfh_modes_many] batch %d: %d modes, set %d, seeded %d, iterations %d, setup %.3f ms, solve %.3f ms\n", r.batches, nb, nqNow, nSeed, lo.iterations, lo.setupMs, lo.solveMs);
        for (int j = 0; j < nb; ++j) r.batchOf[(size_t)(r.found + j)] = r.batches;
        ++r.batches;
        r.iterations += lo.iterations; r.restarts += lo.restarts; r.setupMs += lo.setupMs; r.solveMs += lo.solveMs;
        r.lockDefect = std::max(r.lockDefect, lo.lockDefect);
        r.sign.insert(r.sign.end(), lo.sign.begin(), lo.sign.end());
        MFH_HIP(hipMemcpyAsync(w.col(Q, nqNow), w.X, L * (size_t)nb * sizeof(double), hipMemcpyDeviceToDevice, s));
        for (int j = 0; j < nb; ++j) w.apply_B(w.col(Q, nqNow + j), w.col(BQ, nqNow + j));
        nSeed = useSeed ? lo.blockSize - nb : 0;
        if (nSeed > 0) {
            seed.reserve(L * (size_t)BLK_MAXC);
            MFH_HIP(hipMemcpyAsync(seed.p, w.col(w.X, nb), L * (size_t)nSeed * sizeof(double), hipMemcpyDeviceToDevice, s));
        }
        nqNow += nb; r.found += nb;
        if (!lo.done) { r.allDone = false; break; }
        if (band) {
            for (int j = r.found - nb; j < r.found; ++j) r.exhausted = r.exhausted || lambda[j] > p.lambdaMax;
            if (r.exhausted) break;
        }
    }
}

// The full residuals of everything found, unprojected against what the call itself locked: K x afresh, k_block_residual in groups of the block's
// width. The caller's Q need not be eigenvectors: with them, the residual of the restricted pencil. Returns the device time in ms.
double many_full_residuals(ModesWork &w, double *Q, double *BQ, int nLocked, int found, const double *lambda, double *res) {
    EventTimer tr(w.s);
    const DeflationSet given{Q, BQ, nLocked, nLocked};
    for (int g0 = 0; g0 < found; g0 += w.m) {
        const int kg = std::min(w.m, found - g0);
        for (int j = 0; j < kg; ++j) w.apply_A(w.col(Q, nLocked + g0 + j), w.col(w.KX, j));
        block_residuals(w, &given, kg, lambda + g0, w.KX, w.col(BQ, nLocked + g0), res + g0);
    }
    return tr.stop();
}

// Sorted by lambda (lambda, res and the rows of X, in place); a mode of a later batch that sorts before an earlier batch's largest (by more than
// rtol) is counted and named in the note. Returns that count.
int many_sort(mfh_ctx *c, int64_t n, const ManyRun &r, double rtol, double *lambda, double *res, double *Xout, std::vector<int> &order) {
    const int found = r.found;
    order = iota(found);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lambda[a] < lambda[b]; });
    int nOut = 0;
    std::vector<double> hiOfBatch((size_t)std::max(r.batches, 1), -1e300);
    for (int j = 0; j < found; ++j) hiOfBatch[(size_t)r.batchOf[(size_t)j]] = std::max(hiOfBatch[(size_t)r.batchOf[(size_t)j]], lambda[j]);
    for (int b = 1; b < r.batches; ++b) hiOfBatch[(size_t)b] = std::max(hiOfBatch[(size_t)b], hiOfBatch[(size_t)b - 1]);
    std::string names;
    for (int j = 0; j < found; ++j)
        if (r.batchOf[(size_t)j] > 0 && lambda[j] < hiOfBatch[(size_t)r.batchOf[(size_t)j] - 1] * (1.0 - rtol)) {     // (below by more than rtol: the other member of a multiple eigenvalue that a batch edge cut is no missed mode)
            ++nOut;
            const int pos = (int)(std::find(order.begin(), order.end(), j) - order.begin());
            names += (names.empty() ? "" : ", ") + std::to_string(pos) + " (batch " + std::to_string(r.batchOf[(size_t)j]) + ")";
        }
    if (nOut > 0) modes_note(c, "modes out of order (a later batch found them below an earlier batch's largest; sorted position): " + names);
    std::vector<double> lam2((size_t)found), res2((size_t)found), row((size_t)n);
    for (int j = 0; j < found; ++j) { lam2[(size_t)j] = lambda[order[(size_t)j]]; res2[(size_t)j] = res[(size_t)order[(size_t)j]]; }
    // rows of X in place, cycle by cycle
    std::vector<uint8_t> seen((size_t)found, 0);
    for (int st = 0; st < found; ++st) {
        if (seen[(size_t)st] || order[(size_t)st] == st) { seen[(size_t)st] = 1; continue; }
        std::copy(Xout + (size_t)st * (size_t)n, Xout + (size_t)(st + 1) * (size_t)n, row.begin());
        int at = st;
        for (;;) {
            seen[(size_t)at] = 1;
            const int from = order[(size_t)at];
            if (from == st) { std::copy(row.begin(), row.end(), Xout + (size_t)at * (size_t)n); break; }
            std::copy(Xout + (size_t)from * (size_t)n, Xout + (size_t)(from + 1) * (size_t)n, Xout + (size_t)at * (size_t)n);
            at = from;
        }
    }
    for (int j = 0; j < found; ++j) { lambda[j] = lam2[(size_t)j]; res[(size_t)j] = res2[(size_t)j]; }
    return nOut;
}

void modes_keep_record(mfh_ctx *c, mfh_ctx::ModesKeep &kp, int64_t n, int64_t ld, const std::vector<int> &src, const std::vector<double> &sign, const double *lambda) {
    kp.n = n; kp.ld = ld; kp.src = src; kp.sign = sign;
    kp.lambda.assign(lambda, lambda + src.size());
    kp.fixedSet = c->fixedVars;
    std::sort(kp.fixedSet.begin(), kp.fixedSet.end());
    kp.geoGen = c->geoGen; kp.densityGen = c->densityGen;
}

}   // namespace

extern "C" {

mfh_status mfh_modes(mfh_ctx *c, int32_t nev, double density, int32_t flags, double rtol, int32_t maxit, double *lambda, double *Xout, double *residuals,
                     mfh_modes_info *info) {
    if (info) { *info = mfh_modes_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c && nev >= 1 && nev <= 20 && density > 0.0 && std::isfinite(density) && lambda && Xout && rtol > 0.0 && maxit > 0 && (flags & ~MFH_MODES_FREE) == 0,
            MFH_ERR_INVALID, "mfh_modes: 1 <= nev <= 20, density > 0, rtol > 0, maxit > 0, lambda and X not null");
    require(c->haveMesh && !c->external, MFH_ERR_STATE, "mfh_modes: no mesh set");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    const bool freeBody = (flags & MFH_MODES_FREE) != 0;
    modes_require_context(c, freeBody, "mfh_modes");
    ModesGuard guard(c);
    EventTimer tsetup(c->stream);
    ModesWork w;
    modes_prepare(c, ModesSetup{"mfh_modes", Pencil::Vibration, freeBody, density, 0.0, true, false}, w);
    const LoopIn in{nev, freeBody, rtol, maxit, lambda, Xout, residuals};
    LoopOut lo;
    lobpcg_run(w, in, tsetup, lo);
    modes_fill_info(info, c, w, lo);
    require_converged(lo);
    MFH_CATCH(c)
}

mfh_status mfh_modes_many(mfh_ctx *c, const mfh_modes_many_params *prm, const double *Qin, double *lambda, double *Xout, double *residuals,
                          mfh_modes_many_info *info) {
    if (info) { *info = mfh_modes_many_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c && prm && lambda && Xout, MFH_ERR_INVALID, "mfh_modes_many: context, parameters, lambda and X not null");
    const mfh_modes_many_params p = *prm;
    const int nLocked = p.nLocked, nev = p.nev;
    require(nLocked >= 0 && nLocked <= 255 && nev >= 1 && nev <= 256 - nLocked && p.batch >= 0 && p.batch <= 20 && p.maxit > 0 && p.reserved == 0 &&
                (p.flags & ~MFH_MODES_FREE) == 0,
            MFH_ERR_INVALID, "mfh_modes_many: 0 <= nLocked <= 255, 1 <= nev <= 256 - nLocked, 0 <= batch <= 20, maxit > 0, flags 0 | MFH_MODES_FREE, reserved 0");
    require(p.density > 0.0 && std::isfinite(p.density) && p.rtol > 0.0 && std::isfinite(p.rtol), MFH_ERR_INVALID, "mfh_modes_many: density > 0, rtol > 0");
    const double lockFactor = p.lockFactor == 0.0 ? 0.1 : p.lockFactor;
    require(lockFactor > 0.0 && lockFactor <= 1.0, MFH_ERR_INVALID, "mfh_modes_many: lockFactor in (0, 1] (0: the default 0.1)");
    require(!std::isnan(p.lambdaMax), MFH_ERR_INVALID, "mfh_modes_many: lambdaMax is not a number");
    require(nLocked == 0 || Qin, MFH_ERR_INVALID, "mfh_modes_many: nLocked > 0 needs Q");
    require(c->haveMesh && !c->external, MFH_ERR_STATE, "mfh_modes_many: no mesh set");
    const bool freeBody = (p.flags & MFH_MODES_FREE) != 0;
    const bool band = p.lambdaMax > 0.0 && std::isfinite(p.lambdaMax);
    const int batch = p.batch == 0 ? 16 : p.batch;
    const int64_t n = (int64_t)c->bs() * c->nDoF;
    {
        const int nz = freeBody ? (c->bs() == 3 ? 6 : 3) : 0;
        require((int64_t)nev + nLocked + nz <= n - (int64_t)c->fixedVars.size(), MFH_ERR_INVALID, "mfh_modes_many: nev + nLocked (+ the rigid modes) exceed the dimension of the pencil");
        for (int64_t e = 0; e < (int64_t)nLocked * n; ++e)
            require(std::isfinite(Qin[e]), MFH_ERR_INVALID, "mfh_modes_many: Q has an entry that is not finite");
    }
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    modes_require_context(c, freeBody, "mfh_modes_many");
    hipStream_t s = c->stream;
    ModesGuard guard(c);
    EventTimer tsetup(s);
    ModesWork w;
    modes_prepare(c, ModesSetup{"mfh_modes_many", Pencil::Vibration, freeBody, p.density, 0.0, true, false}, w);
    const int precondUsed = modes_precond_used(c, w);
    if (nLocked == 0 && nev <= batch && !band) {
        // one batch and nothing to deflate: the call of mfh_modes, its bits, its residuals
        const LoopIn in{nev, freeBody, p.rtol, p.maxit, lambda, Xout, residuals};
        LoopOut lo;
        lobpcg_run(w, in, tsetup, lo);
        if (info) {
            info->converged = lo.done ? 1 : 0;
            info->nFound = nev; info->batches = 1; info->iterations = lo.iterations; info->restarts = lo.restarts; info->precondUsed = precondUsed;
            info->maxResidual = lo.maxResidual; info->solve_ms = lo.solveMs; info->setup_ms = lo.setupMs;
            info->note = c->modesNote.c_str();
        }
        require_converged(lo);
        // what mfh_modal_set_basis_from_modes adopts: the block's returned columns
        mfh_ctx::ModesKeep &kp = c->modesKeep;
        kp.reset();
        kp.Q.alloc((size_t)w.ld * (size_t)nev);
        MFH_HIP(hipMemcpyAsync(kp.Q.p, w.X, (size_t)w.ld * (size_t)nev * sizeof(double), hipMemcpyDeviceToDevice, s));
        MFH_HIP(hipStreamSynchronize(s));
        modes_keep_record(c, kp, n, w.ld, iota(nev), lo.sign, lambda);
        return MFH_OK;
    }
    // ---- the deflation set: Q and M Q, nLocked + nev columns each
    const size_t L = (size_t)w.ld;
    DBuf<double> setQ, setBQ;
    setQ.alloc(L * (size_t)(nLocked + nev)); setBQ.alloc(L * (size_t)(nLocked + nev));
    setQ.zero(s); setBQ.zero(s);
    deflate_alloc(w);
    modes_scratch(w);
    w.nz = freeBody ? (w.d == 3 ? 6 : 3) : 0;
    if (nLocked > 0) many_orthonormalise_given(w, freeBody, Qin, nLocked, setQ.p, setBQ.p);
    ManyRun r;
    many_batches(w, p, batch, lockFactor, band, tsetup, setQ.p, setBQ.p, lambda, Xout, r);
    r.solveMs += many_full_residuals(w, setQ.p, setBQ.p, nLocked, r.found, lambda, r.res.data());
    std::vector<int> order;
    const int nOut = many_sort(c, n, r, p.rtol, lambda, r.res.data(), Xout, order);
    int nFound = r.found;
    if (band)
        while (nFound > 0 && lambda[nFound - 1] > p.lambdaMax) --nFound;
    // rows past nFound hold nothing: zero
    for (int j = nFound; j < nev; ++j) { lambda[j] = 0.0; r.res[(size_t)j] = 0.0; }
    std::fill(Xout + (size_t)nFound * (size_t)n, Xout + (size_t)nev * (size_t)n, 0.0);
    double mr = 0;
    for (int j = 0; j < nFound; ++j) mr = std::max(mr, r.res[(size_t)j]);
    if (residuals) std::copy(r.res.begin(), r.res.end(), residuals);
    const bool converged = r.allDone && mr <= p.rtol;
    if (info) {
        info->converged = converged ? 1 : 0;
        info->nFound = nFound; info->batches = r.batches; info->iterations = r.iterations; info->restarts = r.restarts; info->precondUsed = precondUsed;
        info->bandExhausted = r.exhausted ? 1 : 0; info->nOutOfOrder = nOut;
        info->maxResidual = mr; info->maxLockDefect = r.lockDefect; info->solve_ms = r.solveMs; info->setup_ms = r.setupMs;
        info->note = c->modesNote.c_str();
    }
    if (!r.allDone) throw Error(MFH_ERR_NOT_CONVERGED, "LOBPCG did not reach the requested tolerance within maxit iterations (batch " + std::to_string(r.batches - 1) + ")");
    if (!converged) throw Error(MFH_ERR_NOT_CONVERGED, "the full residuals of the locked modes exceed rtol (largest " + std::to_string(mr / p.rtol) + " rtol): lower lockFactor");
    {   // the set stays for mfh_modal_set_basis_from_modes instead of being freed here: sorted mode j is its column nLocked + order[j]
        mfh_ctx::ModesKeep &kp = c->modesKeep;
        kp.reset();
        MFH_HIP(hipStreamSynchronize(s));
        kp.Q.swap(setQ);
        std::vector<int> src((size_t)nFound);
        std::vector<double> sg((size_t)nFound);
        for (int j = 0; j < nFound; ++j) { src[(size_t)j] = nLocked + order[(size_t)j]; sg[(size_t)j] = r.sign[(size_t)order[(size_t)j]]; }
        modes_keep_record(c, kp, n, w.ld, src, sg, lambda);
    }
    MFH_CATCH(c)
}

}   // extern "C"

// ---------------------------------------------------------------- linear buckling (docs/design/04_16_buckling.md)
namespace {
// the contexts a prestress field is defined on: those of mfh_set_density
void require_prestress_context(mfh_ctx *c, const char *who) {
    if (!c) throw Error(MFH_ERR_INVALID, std::string(who) + ": null context");
    require(c->haveMesh && !c->hostOnly && !c->external, MFH_ERR_STATE, "the prestress field needs a mesh on a device");
    if (!(!dist_active(c) && c->mesh.nOwned == c->mesh.nNode && c->nOwnedDoF() == c->nDoF)) throw Error(MFH_ERR_UNSUPPORTED, std::string(who) + ": unpartitioned contexts only");
    require(c->mesh.dim == 2 || c->mesh.dim == 3, MFH_ERR_UNSUPPORTED, "2D / 3D meshes");
}
// ... and those Kg is defined on: the elasticity operator on the mesh's own degree (the conditions of mfh_modes)
void require_geometric_context(mfh_ctx *c, const char *who) {
    require_prestress_context(c, who);
    if (!(c->op == MFH_OP_ELASTICITY && c->opDegree != 1))
        throw Error(MFH_ERR_UNSUPPORTED, std::string(who) + ": the pencil is (geometric stiffness, elasticity) on the mesh's own degree: select MFH_OP_ELASTICITY and leave the forced-degree-1 view");
    if (!c->havePrestress) throw Error(MFH_ERR_STATE, std::string(who) + ": no prestress field set (mfh_set_prestress / mfh_prestress_from_displacement)");
}
}   // namespace

extern "C" {

mfh_status mfh_set_prestress(mfh_ctx *c, const double *sigma, int64_t n, int32_t flags) {
    MFH_TRY(c)
    require_prestress_context(c, "mfh_set_prestress");
    require((flags & ~MFH_LOAD_ON_DEVICE) == 0, MFH_ERR_INVALID, "flags: 0 | MFH_LOAD_ON_DEVICE");
    if (!sigma) {
        if (c->havePrestress) clear_prestress(c);
        return MFH_OK;
    }
    const int64_t nElem = c->mesh.nElem, fl = flat_len(c->mesh.dim), count = nElem * fl;
    require(n == nElem, MFH_ERR_INVALID, "mfh_set_prestress: one symmetric tensor (flatLen values) per element");
    const bool onDevice = (flags & MFH_LOAD_ON_DEVICE) != 0;
    MFH_HIP(hipSetDevice(c->device));
    bool bad = false;
    if (!onDevice) {
        for (int64_t q = 0; q < count && !bad; ++q) bad = !std::isfinite(sigma[q]);
    } else {
        DBuf<int> flag;
        flag.alloc(1);
        flag.zero(c->stream);
        k::launch_prestress_finite(count, sigma, flag.p, c->stream);
        int h = 0;
        flag.download(&h, 1, c->stream);
        bad = h != 0;
    }
    require(!bad, MFH_ERR_INVALID, "mfh_set_prestress: an entry is not finite");
    // a buffer of its own every time: the field in force stays untouched until the new one is complete
    DBuf<double> fresh;
    fresh.alloc((size_t)count);
    MFH_HIP(hipMemcpyAsync(fresh.p, sigma, (size_t)count * sizeof(double), onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    MFH_HIP(hipStreamSynchronize(c->stream));
    c->dPrestress.swap(fresh);
    c->havePrestress = true;
    ++c->prestressGen;
    MFH_CATCH(c)
}

// sigma_e = C_e : (element-average strain of u), written by k_average_strain into a fresh buffer of the context
mfh_status mfh_prestress_from_displacement(mfh_ctx *c, const double *uNodes, int32_t flags) {
    MFH_TRY(c)
    require_prestress_context(c, "mfh_prestress_from_displacement");
    require(uNodes != nullptr, MFH_ERR_INVALID, "mfh_prestress_from_displacement: null displacement");
    require((flags & ~MFH_LOAD_ON_DEVICE) == 0, MFH_ERR_INVALID, "flags: 0 | MFH_LOAD_ON_DEVICE");
    require(c->op == MFH_OP_ELASTICITY && c->opDegree != 1, MFH_ERR_UNSUPPORTED, "mfh_prestress_from_displacement: the stress field is defined for the elasticity operator on the mesh's own degree");
    MFH_HIP(hipSetDevice(c->device));
    const bool onDevice = (flags & MFH_LOAD_ON_DEVICE) != 0;
    const HostMesh &m = c->mesh;
    const int d = m.dim, fl = flat_len(d);
    const size_t nu = (size_t)m.nNode * d;
    if (!onDevice)
        for (size_t q = 0; q < nu; ++q) require(std::isfinite(uNodes[q]), MFH_ERR_INVALID, "mfh_prestress_from_displacement: an entry is not finite");
    ensure_geometry(c);
    DBuf<double> du, fresh;
    DBuf<int> flag;
    const double *u = uNodes;
    if (!onDevice) {
        du.alloc(nu);
        MFH_HIP(hipMemcpyAsync(du.p, uNodes, nu * sizeof(double), hipMemcpyHostToDevice, c->stream));
        u = du.p;
    }
    fresh.alloc((size_t)m.nElem * fl);
    k::launch_average_strain(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), u, fresh.p, 1, nullptr, nullptr, c->stream);
    flag.alloc(1);
    flag.zero(c->stream);
    k::launch_prestress_finite((int64_t)m.nElem * fl, fresh.p, flag.p, c->stream);
    int h = 0;
    flag.download(&h, 1, c->stream);
    require(h == 0, MFH_ERR_INVALID, "mfh_prestress_from_displacement: the stress of this displacement is not finite");
    c->dPrestress.swap(fresh);
    c->havePrestress = true;
    ++c->prestressGen;
    MFH_CATCH(c)
}

// the nev smallest load factors of (K + factor Kg) x = 0: the loop of mfh_modes on the pencil (Kg, K); K's preconditioner approximates B^-1 here
mfh_status mfh_buckling(mfh_ctx *c, int32_t nev, int32_t flags, double rtol, int32_t maxit, double *factors, double *Xout, double *residuals,
                        mfh_buckling_info *info) {
    if (info) { *info = mfh_buckling_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c && nev >= 1 && nev <= 20 && factors && Xout && rtol > 0.0 && maxit > 0 && flags == 0, MFH_ERR_INVALID,
            "mfh_buckling: 1 <= nev <= 20, flags 0, rtol > 0, maxit > 0, factors and X not null");
    require_geometric_context(c, "mfh_buckling");
    MFH_HIP(hipSetDevice(c->device));
    {
        const int q = free_rigid_motions(c);
        if (q > 0) throw Error(MFH_ERR_UNSUPPORTED, "the fixed variables leave " + std::to_string(q) + " rigid motions free: K is singular there and the pencil (Kg, K) undefined (fix more variables)");
    }
    require(nev <= (int64_t)c->bs() * c->nDoF - (int64_t)c->fixedVars.size(), MFH_ERR_INVALID, "mfh_buckling: more modes asked for than the pencil has");
    ModesGuard guard(c);
    EventTimer tsetup(c->stream);
    ModesWork w;
    modes_prepare(c, ModesSetup{"mfh_buckling", Pencil::Buckling, false, 1.0, 0.0, false, true}, w);
    std::vector<double> mu((size_t)nev, 0.0);
    const LoopIn in{nev, false, rtol, maxit, mu.data(), Xout, residuals};
    LoopOut lo;
    lobpcg_run(w, in, tsetup, lo);
    // mu ascending; a load factor exists where mu is negative beyond rounding
    double muMax = 0.0;
    for (int j = 0; j < nev; ++j) muMax = std::max(muMax, std::fabs(mu[(size_t)j]));
    int nNeg = 0;
    for (int j = 0; j < nev; ++j) {
        if (mu[(size_t)j] >= -1e-12 * muMax) factors[j] = INFINITY;
        else { factors[j] = -1.0 / mu[(size_t)j]; ++nNeg; }
    }
    modes_fill_info(info, c, w, lo);
    if (info) info->nBuckling = nNeg;
    require_converged(lo);
    MFH_CATCH(c)
}

// ---------------------------------------------------------------- prestressed vibration (docs/design/04_18_prestressed_modes.md)
// the smallest eigenpairs of (K + loadFactor Kg) x = lambda density M x: the loop of mfh_modes on its third pencil, K's preconditioner (the
// shifted operator has none of its own)
mfh_status mfh_modes_prestressed(mfh_ctx *c, int32_t nev, double density, double loadFactor, int32_t flags, double rtol, int32_t maxit, const double *X0,
                                 double *lambda, double *Xout, double *residuals, mfh_modes_info *info) {
    if (info) { *info = mfh_modes_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c && nev >= 1 && nev <= 20 && density > 0.0 && std::isfinite(density) && std::isfinite(loadFactor) && lambda && Xout && rtol > 0.0 && maxit > 0,
            MFH_ERR_INVALID, "mfh_modes_prestressed: 1 <= nev <= 20, density > 0, a finite load factor, rtol > 0, maxit > 0, lambda and X not null");
    require(flags == 0, MFH_ERR_UNSUPPORTED,
            "mfh_modes_prestressed: rigid rotations are not in the kernel of Kg, so the known-kernel variant (MFH_MODES_FREE) does not apply");
    require(c->haveMesh && !c->external, MFH_ERR_STATE, "mfh_modes_prestressed: no mesh set");
    require_geometric_context(c, "mfh_modes_prestressed");
    MFH_HIP(hipSetDevice(c->device));
    {
        const int q = free_rigid_motions(c);
        if (q > 0) throw Error(MFH_ERR_UNSUPPORTED, "the fixed variables leave " + std::to_string(q) + " rigid motions free: the clamped pencil is singular (fix more variables)");
    }
    const int64_t nAll = (int64_t)c->bs() * c->nDoF;
    require(nev <= nAll - (int64_t)c->fixedVars.size(), MFH_ERR_INVALID, "mfh_modes_prestressed: more modes asked for than the pencil has");
    if (X0)
        for (int64_t q = 0; q < (int64_t)nev * nAll; ++q) require(std::isfinite(X0[q]), MFH_ERR_INVALID, "mfh_modes_prestressed: an entry of X0 is not finite");
    ModesGuard guard(c);
    EventTimer tsetup(c->stream);
    ModesWork w;
    modes_prepare(c, ModesSetup{"mfh_modes_prestressed", Pencil::Prestressed, false, density, loadFactor, true, true}, w);
    LoopIn in{nev, false, rtol, maxit, lambda, Xout, residuals};
    in.X0 = X0;
    LoopOut lo;
    lobpcg_run(w, in, tsetup, lo);
    int nNeg = 0;
    for (int j = 0; j < nev; ++j) nNeg += lambda[j] < 0.0 ? 1 : 0;
    if (nNeg > 0) modes_note(c, std::to_string(nNeg) + " of the " + std::to_string(nev) + " eigenvalues are negative: the prestressed state is unstable at this load factor");
    modes_fill_info(info, c, w, lo);
    require_converged(lo);
    MFH_CATCH(c)
}

// test hook (meshfem_hip_extras.h; tests/test_gpu_lobpcg_iterates.py): lobpcg_run itself on a pencil of the caller's choice, from a whole start
// block of the caller's, with an optional deflation set, and its history (LoopTrace). The checks are those of the entry point of the pencil.
mfh_status mfh_debug_lobpcg(mfh_ctx *c, int32_t pencil, double density, double loadFactor, int32_t freeBody, int32_t nev, double rtol, int32_t maxit, int32_t m,
                            const double *S0, int32_t nq, const double *Q, int32_t *blockSize, double *X, double *lambdaHist, double *resHist, int32_t *sets,
                            int32_t *iterations, int32_t *precondUsed) {
    MFH_TRY(c)
    require(c && pencil >= 0 && pencil <= 2 && nev >= 1 && nev <= 20 && density > 0.0 && std::isfinite(density) && std::isfinite(loadFactor) && rtol > 0.0 && maxit >= 0 &&
                nq >= 0 && nq <= k::DEFL_MAXQ && blockSize,
            MFH_ERR_INVALID, "mfh_debug_lobpcg: arguments");
    require(c->haveMesh && !c->external, MFH_ERR_STATE, "mfh_debug_lobpcg: no mesh set");
    const Pencil kind = pencil == 0 ? Pencil::Vibration : (pencil == 1 ? Pencil::Buckling : Pencil::Prestressed);
    const bool fb = freeBody != 0;
    require(kind == Pencil::Vibration || !fb, MFH_ERR_UNSUPPORTED, "mfh_debug_lobpcg: the free body is a case of the vibration pencil");
    if (kind == Pencil::Vibration) {
        require_device(c);
        MFH_HIP(hipSetDevice(c->device));
        modes_require_context(c, fb, "mfh_debug_lobpcg");
    } else {
        require_geometric_context(c, "mfh_debug_lobpcg");
        MFH_HIP(hipSetDevice(c->device));
        require(free_rigid_motions(c) == 0, MFH_ERR_UNSUPPORTED, "mfh_debug_lobpcg: the fixed variables leave rigid motions free");
    }
    const int64_t n = (int64_t)c->bs() * c->nDoF;
    const int64_t nEff = n - (int64_t)c->fixedVars.size() - (fb ? (c->bs() == 3 ? 6 : 3) : 0) - nq;
    require(nev <= nEff, MFH_ERR_INVALID, "mfh_debug_lobpcg: more modes asked for than the pencil has");
    *blockSize = Lobpcg::block_size(nev, nEff);
    if (!S0) return MFH_OK;                        // (the question alone: how many rows does S0 take)
    require(m == *blockSize, MFH_ERR_INVALID, "mfh_debug_lobpcg: S0 takes as many rows as the loop's block has columns (*blockSize)");
    require(X && lambdaHist && resHist && sets && iterations && precondUsed && (nq == 0 || Q), MFH_ERR_INVALID, "mfh_debug_lobpcg: null output, or nq > 0 without Q");
    for (int64_t q = 0; q < (int64_t)m * n; ++q) require(std::isfinite(S0[q]), MFH_ERR_INVALID, "mfh_debug_lobpcg: an entry of S0 is not finite");
    for (int64_t q = 0; q < (int64_t)nq * n; ++q) require(std::isfinite(Q[q]), MFH_ERR_INVALID, "mfh_debug_lobpcg: an entry of Q is not finite");
    ModesGuard guard(c);
    EventTimer tsetup(c->stream);
    ModesWork w;
    const bool vib = kind == Pencil::Vibration;
    modes_prepare(c, ModesSetup{"mfh_debug_lobpcg", kind, fb, vib || kind == Pencil::Prestressed ? density : 1.0, kind == Pencil::Prestressed ? loadFactor : 0.0,
                                kind != Pencil::Buckling, !vib}, w);
    *precondUsed = modes_precond_used(c, w);
    // the deflation set as the caller gives it (B-orthonormal), with its B-image
    DBuf<double> setQ, setBQ;
    DeflationSet ds;
    if (nq > 0) {
        const size_t L = (size_t)w.ld;
        setQ.alloc(L * (size_t)nq); setBQ.alloc(L * (size_t)nq);
        setQ.zero(w.s); setBQ.zero(w.s);
        deflate_alloc(w);
        MFH_HIP(hipMemcpy2DAsync(setQ.p, L * sizeof(double), Q, (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)nq, hipMemcpyHostToDevice, w.s));
        MFH_HIP(hipStreamSynchronize(w.s));
        for (int j = 0; j < nq; ++j) w.apply_B(w.col(setQ.p, j), w.col(setBQ.p, j));
        ds = DeflationSet{setQ.p, setBQ.p, nq, nq};
    }
    std::vector<double> lam((size_t)nev), Xret((size_t)nev * (size_t)n), res((size_t)nev);
    LoopTrace trace;
    trace.X = X;
    LoopIn in{nev, fb, rtol, maxit, lam.data(), Xret.data(), res.data()};
    in.X0 = S0; in.nX0 = m;
    if (nq > 0) in.defl = &ds;
    in.trace = &trace;
    LoopOut lo;
    lobpcg_run(w, in, tsetup, lo);
    const size_t calls = trace.sets.size() / 3;
    std::copy(trace.lam.begin(), trace.lam.end(), lambdaHist);
    std::copy(trace.res.begin(), trace.res.end(), resHist);
    std::copy(trace.sets.begin(), trace.sets.end(), sets);
    for (size_t q = calls * (size_t)m; q < (size_t)(maxit + 1) * (size_t)m; ++q) lambdaHist[q] = resHist[q] = NAN;   // (the calls a stop spared)
    for (size_t q = calls * 3; q < (size_t)(maxit + 1) * 3; ++q) sets[q] = -1;
    *iterations = lo.done ? lo.iterations : -1;
    require_converged(lo);
    MFH_CATCH(c)
}

// y = (K + loadFactor Kg) x on displacement vectors, unmasked: the context's operator, then the accumulate pass on the geometric buffer
mfh_status mfh_tangent_apply(mfh_ctx *c, double loadFactor, const double *x, double *y, int32_t flags) {
    MFH_TRY(c)
    require(c && x && y && std::isfinite(loadFactor), MFH_ERR_INVALID, "mfh_tangent_apply: null argument or a load factor that is not finite");
    require((flags & ~MFH_LOAD_ON_DEVICE) == 0, MFH_ERR_INVALID, "flags: 0 | MFH_LOAD_ON_DEVICE");
    require(c->haveMesh && !c->hostOnly && !c->external, MFH_ERR_STATE, "the tangent stiffness needs a mesh on a device");
    prepare_pencil(c, "mfh_tangent_apply");
    require(c->havePrestress, MFH_ERR_STATE, "mfh_tangent_apply: no prestress field set (mfh_set_prestress / mfh_prestress_from_displacement)");
    hipStream_t s = c->stream;
    WideGuard guard(c);
    ensure_precond(c);                 // (K assembled, the fixed-variable mask on the device)
    require(c->sym.nRows == c->sym.nCols, MFH_ERR_UNSUPPORTED, "mfh_tangent_apply: unpartitioned contexts only");
    ensure_geometric(c);
    prepare_matrix_free(c);
    if (!c->use_mf()) require_full_storage(c, "the assembled SpMV of mfh_tangent_apply");
    const bool onDevice = (flags & MFH_LOAD_ON_DEVICE) != 0;
    const int64_t n = (int64_t)c->bs() * c->nDoF;
    DBuf<double> dx, dy;
    const double *xin = x;
    double *yout = y;
    if (!onDevice) {
        dx.alloc((size_t)n); dy.alloc((size_t)n);
        upload(dx.p, x, n, s);
        xin = dx.p; yout = dy.p;
    }
    apply_operator(c, false, xin, yout, nullptr);
    k::launch_spmv_kron_acc(geom_spmv_args(c, false), true, 1.0, loadFactor, xin, yout, nullptr, k::DynGate{nullptr, 0, nullptr}, s);
    if (!onDevice) MFH_HIP(hipMemcpyAsync(y, dy.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

// test hook (meshfem_hip_extras.h): the pair product as the prestressed loop launches it, on host vectors; twoPass forces the two-launch form
mfh_status mfh_debug_kron_pair(mfh_ctx *c, double sG, double rho, int32_t masked, int32_t twoPass, const double *x, double *yA, double *yB) {
    MFH_TRY(c)
    require(c && x && yA && yB && std::isfinite(sG) && std::isfinite(rho), MFH_ERR_INVALID, "mfh_debug_kron_pair: arguments");
    require(c->haveMesh && !c->hostOnly && !c->external, MFH_ERR_STATE, "the pair product needs a mesh on a device");
    prepare_pencil(c, "mfh_debug_kron_pair");
    require(c->havePrestress, MFH_ERR_STATE, "mfh_debug_kron_pair: no prestress field set");
    hipStream_t s = c->stream;
    WideGuard guard(c);
    ensure_fixed_uploaded(c);
    ensure_mass(c);
    ensure_geometric(c);
    const int64_t n = (int64_t)c->bs() * c->nDoF;
    const bool m = masked != 0 && !c->fixedVars.empty();
    DBuf<double> dx, da, db;
    dx.alloc((size_t)n); da.alloc((size_t)n); db.alloc((size_t)n);
    upload(dx.p, x, n, s);
    upload(da.p, yA, n, s);
    k::launch_spmv_kron_pair(mass_spmv_args(c, m), c->dGeomVals.p, c->dMassVals.p, sG, rho, dx.p, da.p, db.p, n, twoPass != 0, s);
    MFH_HIP(hipMemcpyAsync(yA, da.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(yB, db.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    MFH_CATCH(c)
}

// measurement (meshfem_hip_extras.h): average device time of `reps` pair products on hashed vectors in the single pass and in the two-launch form
// (density 1, the default of every facade: the two-launch form then pays no scaling kernel), in alternating groups after a warm-up of both
mfh_status mfh_time_kron_pair(mfh_ctx *c, int32_t reps, double *pair_ms, double *separate_ms) {
    MFH_TRY(c)
    require(c && pair_ms && separate_ms && reps > 0, MFH_ERR_INVALID, "bad arguments");
    require(c->haveMesh && !c->hostOnly && !c->external, MFH_ERR_STATE, "the pair product needs a mesh on a device");
    prepare_pencil(c, "mfh_time_kron_pair");
    require(c->havePrestress, MFH_ERR_STATE, "mfh_time_kron_pair: no prestress field set");
    hipStream_t s = c->stream;
    WideGuard guard(c);
    ensure_fixed_uploaded(c);
    ensure_mass(c);
    ensure_geometric(c);
    const int64_t n = (int64_t)c->bs() * c->nDoF;
    const k::SpmvArgs a = mass_spmv_args(c, !c->fixedVars.empty());
    DBuf<double> v;
    v.alloc((size_t)3 * n);
    k::launch_fill_hash(3 * n, v.p, s);
    double *x = v.p, *yA = v.p + n, *yB = v.p + 2 * n;
    const int groups = 4, per = (reps + groups - 1) / groups;
    double t[2] = {0.0, 0.0};
    for (int g = -1; g < groups; ++g)          // (g == -1: the warm-up)
        for (int form = 0; form < 2; ++form) {
            EventTimer tm(s);
            for (int r = 0; r < per; ++r) k::launch_spmv_kron_pair(a, c->dGeomVals.p, c->dMassVals.p, 1e-3, 1.0, x, yA, yB, n, form == 1, s);
            const double ms = tm.stop();
            if (g >= 0) t[form] += ms;
        }
    *pair_ms = t[0] / (groups * per);
    *separate_ms = t[1] / (groups * per);
    MFH_CATCH(c)
}

// measurement (meshfem_hip_extras.h): the gather assembly pass into the resident one-double-per-block buffer as the Laplacian (MAT_LAPLACE), the
// unit-density mass (MAT_MASS) and the geometric stiffness of the prestress in force (MAT_GEOM) in the context's own flavour, and MAT_GEOM in the
// turn-taking flavour that ensure_geometric launches, in turns
mfh_status mfh_time_geometric_assembly(mfh_ctx *c, int32_t reps, double *laplace_ms, double *mass_ms, double *geom_ms, double *geom_det_ms) {
    MFH_TRY(c)
    require(c && laplace_ms && mass_ms && geom_ms && geom_det_ms && reps > 0, MFH_ERR_INVALID, "bad arguments");
    require_geometric_context(c, "mfh_time_geometric_assembly");
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometric(c);                         // geometry, pattern (both triangles: option matrix_storage 0), the buffer
    k::AsmArgs a = asm_args(c);
    a.vals = c->dGeomVals.p;
    const int det = a.det;
    for (int r = 0; r < reps; ++r) {
        a.mat = MAT_LAPLACE; a.sigma = nullptr; a.det = det;
        { EventTimer t(c->stream); k::launch_assemble_gather(a, c->stream); laplace_ms[r] = t.stop(); }
        a.mat = MAT_MASS;
        { EventTimer t(c->stream); k::launch_assemble_gather(a, c->stream); mass_ms[r] = t.stop(); }
        a.mat = MAT_GEOM; a.sigma = c->dPrestress.p;
        { EventTimer t(c->stream); k::launch_assemble_gather(a, c->stream); geom_ms[r] = t.stop(); }
        a.det = 1;                               // (last: the buffer is left as ensure_geometric would leave it)
        { EventTimer t(c->stream); k::launch_assemble_gather(a, c->stream); geom_det_ms[r] = t.stop(); }
    }
    MFH_CATCH(c)
}

}   // extern "C"
