// What the loops of mfh_dynamics.hip (real coefficients, PCG) and mfh_harmonic.hip (complex coefficients, COCG) on the pencil operator A = cK K + cM M
// share. Device side: the iteration gate, the two-stage ordered sums, the accumulating mass product and the inverse diagonal blocks of the pencil.
// Host side: the context conditions and device state (prepare_pencil, prepare_pencil_state), the base of the two work structs with its setup and
// choice of preconditioner (PencilWork, setup_pencil_work), and the driver of both loops: batches, read-back, stopping rule (pencil_loop).
// Everything here has internal linkage (anonymous namespaces): each translation unit carries its own copy of the kernels. Not part of the ABI.
// mfh_modes.hip includes it too, for the accumulate pass of its prestressed pencil (K + s Kg: k_spmv_kron_acc on the geometric buffer) and the LDS
// limit of its pair kernel; it takes none of the host side.
//   k_spmv_kron_acc    y = cK y + cM (M (x) I) x: k_spmv_kron's chunks and LDS partials, ADDING into the K product that apply_operator left in y
//                      (cK == 0: y is not read), the fixed rows zeroed, x . y summed per workgroup in the same pass
//   k_pencil_dinv      inverse diagonal blocks of A: cK K_ii + cM m_ii I (fixed rows / columns replaced by the identity), symmetric-packed
// Sums: every producing kernel leaves ONE partial per workgroup and sum (plain stores); k_dyn_reduce adds them in a fixed order (runs of consecutive
// workgroups per lane, then an ordered two-level tree) and stores the total where the loop reads it. No floating-point atomics; the grids depend on n (and option dyn_grid_cap) only, so two
// calls add in the same order.
// Gate: the kernels of iteration `it` are no-ops once scal[4 it + 2] = r.r has met stop[0] (the idiom of the loops in mfh_solver.cpp; the layout of
// the history -- {r.z, p.Ap, r.r, -} per iteration -- and of the control block is theirs, so that mg_precond's kernels take the same gate).
#pragma once
#include "mfh_ctx.hh"
#include "mfh_device.hh"
#include "mfh_dispatch.hh"

namespace mfh { namespace k {

namespace {

constexpr int DYN_GRID_CAP = 2048;      // workgroups of k_spmv_kron_acc (k_spmv_kron's cap) and of the PCG's vector kernels at most = rows of the partials buffer
constexpr int DYN_STEP_CAP = 256;       // workgroups of the three step kernels (once per step: one workgroup per CU is plenty)
constexpr int DYN_NV = 4;               // sums a kernel may emit (stride of the partials)
constexpr size_t HARM_LDS_MAX = 160 * 1024;     // what a workgroup of gfx950 can be granted (launch_k asks for anything above 64 KB): the two-plane
                                                // kernels (k_spmv_kron_cacc, k_spmv_kron_pair) fall back to two launches above it

struct DynGate { const double *scal; int it; const double *stop; };
DynGate dyn_open() { return DynGate{nullptr, 0, nullptr}; }       // the gate of a launch outside the iterations: never closed
DEV bool dyn_closed(const DynGate &g) {
    if (!g.scal) return false;
    const int it = g.it + (int)g.stop[3];
    return it >= 0 && g.scal[(int64_t)it * 4 + 2] <= g.stop[0];
}

// the workgroup's sums (valid in thread 0 after block_sum) -> its row of the partials
template <int NV> DEV void store_partials(double (&v)[NV], double *lds, double *__restrict__ partials) {
    block_sum<NV>(v, lds);
    if (threadIdx.x == 0 && partials) {
#pragma unroll
        for (int k = 0; k < NV; ++k) partials[(int64_t)blockIdx.x * DYN_NV + k] = v[k];
    }
}

// second stage, in a fixed order that depends on nPart alone: lane l adds the G = ceil(nPart / 256) consecutive partials [l G, (l + 1) G) in workgroup
// order, 16 lanes add 16 consecutive lane sums each, one lane adds those 16: dst[t] = scale[t] x the total of column col[t]. (One lane adding 2 048
// partials one dependent load after the other took 0.3 ms, a tenth of a PCG iteration.)
struct ReduceArgs {
    int nPart, nv;
    int col[DYN_NV];
    double scale[DYN_NV];
    double *dst[DYN_NV];
};
__global__ void __launch_bounds__(256) k_dyn_reduce(ReduceArgs a, const double *__restrict__ partials, DynGate g) {
    __shared__ double lane_sum[256], group_sum[16];
    if (dyn_closed(g)) return;          // (uniform over the workgroup)
    const int l = threadIdx.x;
    const int G = (a.nPart + 255) / 256;
    for (int t = 0; t < a.nv; ++t) {
        if (!a.dst[t]) continue;        // (uniform)
        double v = 0.0;
        const int b1 = min((l + 1) * G, a.nPart);
        for (int b = l * G; b < b1; ++b) v += partials[(int64_t)b * DYN_NV + a.col[t]];
        lane_sum[l] = v;
        __syncthreads();
        if (l < 16) {
            double w = 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j) w += lane_sum[l * 16 + j];
            group_sum[l] = w;
        }
        __syncthreads();
        if (l == 0) {
            double w = 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j) w += group_sum[j];
            *a.dst[t] = a.scale[t] * w;
        }
        __syncthreads();
    }
}

// y[N i + c] = cK y[N i + c] + cM sum_j m_ij x[N j + c] (ACC; else cM sum_j ... alone), zero on the fixed rows; partials[blockIdx.x][0] = x . y
// over the workgroup's rows. The chunk walk and the LDS partials are k_spmv_kron's (mfh_kernels.hip): the lanes take consecutive stored blocks,
// then one lane per scalar row adds the row's partials in slot order.
template <int N, bool ACC>
__global__ void __launch_bounds__(256) k_spmv_kron_acc(SpmvArgs a, double cK, double cM, const double *__restrict__ x, double *y,
                                                      double *__restrict__ partials, DynGate g) {
    extern __shared__ __attribute__((aligned(16))) double part[];  // [N][chunkSlots] + 16
    const int CS = a.chunkSlots;
    double *red = part + N * CS;
    if (dyn_closed(g)) return;
    double dot[1] = {0.0};
    for (int64_t chunk = blockIdx.x; chunk < a.nChunk; chunk += gridDim.x) {
        const int r0 = a.chunkRow[chunk], r1 = a.chunkRow[chunk + 1];
        const int s0 = a.rowPtr[r0];
        const int ns = a.rowPtr[r1] - s0;
        for (int t = threadIdx.x; t < ns; t += 256) {
            const int64_t s = (int64_t)s0 + t;
            const int64_t col = a.colIdx[s];
            const double m = a.vals[tiled_index(s, 0, 1)];
#pragma unroll
            for (int c = 0; c < N; ++c) part[c * CS + t] = m * x[col * N + c];
        }
        __syncthreads();
        const int nscalar = (r1 - r0) * N;
        for (int idx = threadIdx.x; idx < nscalar; idx += 256) {
            const int rl = idx / N, c = idx - rl * N;
            const int64_t r = r0 + rl;
            const int b = a.rowPtr[r] - s0, e = a.rowPtr[r + 1] - s0;
            double v = 0;
            for (int t = b; t < e; ++t) v += part[c * CS + t];
            const int64_t gi = r * N + c;
            v *= cM;
            if (ACC) v = fma(cK, y[gi], v);
            if (a.fixedMask && a.fixedMask[gi]) v = 0.0;
            y[gi] = v;
            dot[0] = fma(v, x[gi], dot[0]);
        }
        __syncthreads();
    }
    store_partials<1>(dot, red, partials);
}

template <int DIM> DEV void sym_block_inverse(const double *A, double *Inv) {
    if (DIM == 2) {
        const double det = A[0] * A[3] - A[1] * A[2];
        Inv[0] = A[3] / det; Inv[1] = -A[1] / det; Inv[2] = -A[2] / det; Inv[3] = A[0] / det;
    } else {
        const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
        const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
        Inv[0] = c00 / det; Inv[1] = (A[2] * A[7] - A[1] * A[8]) / det; Inv[2] = (A[1] * A[5] - A[2] * A[4]) / det;
        Inv[3] = c01 / det; Inv[4] = (A[0] * A[8] - A[2] * A[6]) / det; Inv[5] = (A[2] * A[3] - A[0] * A[5]) / det;
        Inv[6] = c02 / det; Inv[7] = (A[1] * A[6] - A[0] * A[7]) / det; Inv[8] = (A[0] * A[4] - A[1] * A[3]) / det;
    }
}

// Inverse diagonal blocks of the pencil operator, in the layout of k_diag_inv (symmetric-packed, flat_idx): cK K_rr + cM m_rr I with the rows and
// columns of fixed variables replaced by the identity. kVals: K's tiled dense blocks (null with cK == 0), mVals: one value per block; both on
// the pattern (rowPtr, colIdx), whose columns are sorted within a row.
template <int DIM>
__global__ void __launch_bounds__(256) k_pencil_dinv(int64_t nRows, const int32_t *__restrict__ rowPtr, const int32_t *__restrict__ colIdx,
                                                    const double *__restrict__ kVals, const double *__restrict__ mVals, double cK, double cM,
                                                    const uint8_t *__restrict__ fixedMask, double *__restrict__ dinv) {
    constexpr int NB = DIM * DIM, NS = DIM * (DIM + 1) / 2;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nRows; r += (int64_t)gridDim.x * 256) {
        double A[NB], Inv[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) A[c] = (c % (DIM + 1) == 0) ? 1.0 : 0.0;
        int lo = rowPtr[r], hi = rowPtr[r + 1];
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            const int cv = colIdx[mid];
            if (cv == r) {
                const double mrr = cM * mVals[tiled_index(mid, 0, 1)];
#pragma unroll
                for (int c = 0; c < NB; ++c) A[c] = (kVals ? cK * kVals[tiled_index(mid, c, NB)] : 0.0) + ((c % (DIM + 1) == 0) ? mrr : 0.0);
                break;
            }
            if (cv < r) lo = mid + 1; else hi = mid;
        }
        if (fixedMask) {
#pragma unroll
            for (int c = 0; c < DIM; ++c)
                if (fixedMask[r * DIM + c]) {
#pragma unroll
                    for (int d = 0; d < DIM; ++d) { A[c * DIM + d] = 0.0; A[d * DIM + c] = 0.0; }
                    A[c * DIM + c] = 1.0;
                }
        }
        sym_block_inverse<DIM>(A, Inv);
        // the identity on the fixed variables EXACTLY: with one fixed component of three, the cofactor and the determinant of its diagonal entry are
        // the same 2 x 2 expression contracted into fmas two different ways, and their quotient came out as 1 -+ 1 ulp
        if (fixedMask) {
#pragma unroll
            for (int c = 0; c < DIM; ++c)
                if (fixedMask[r * DIM + c]) {
#pragma unroll
                    for (int d = 0; d < DIM; ++d) { Inv[c * DIM + d] = 0.0; Inv[d * DIM + c] = 0.0; }
                    Inv[c * DIM + c] = 1.0;
                }
        }
#pragma unroll
        for (int c = 0; c < DIM; ++c)
#pragma unroll
            for (int d = c; d < DIM; ++d) dinv[r * NS + flat_idx<DIM>(c, d)] = 0.5 * (Inv[c * DIM + d] + Inv[d * DIM + c]);
    }
}

template <int DIM> DEV void apply_packed(const double *__restrict__ Dm, const double *r, double *z) {
    constexpr int NS = DIM * (DIM + 1) / 2;
    double m[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) m[q] = Dm[q];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
        double v = 0;
#pragma unroll
        for (int d = 0; d < DIM; ++d) v += m[flat_idx<DIM>(c, d)] * r[d];
        z[c] = v;
    }
}

int dyn_grid(int64_t n, int cap = DYN_STEP_CAP) { return grid_for(n, cap); }

void launch_reduce(int nPart, int nv, const int *col, const double *scale, double *const *dst, const double *partials, const DynGate &g, hipStream_t s) {
    ReduceArgs a{};
    a.nPart = nPart; a.nv = nv;
    for (int t = 0; t < nv; ++t) { a.col[t] = col[t]; a.scale[t] = scale[t]; a.dst[t] = dst[t]; }
    hipLaunchKernelGGL(k_dyn_reduce, dim3(1), dim3(256), 0, s, a, partials, g);
    CHECK_LAUNCH();
}

// the usual sums: the totals of columns 0[, 1[, 2]] as they are, to dst0[, dst1[, dst2]] (a null destination is skipped)
void launch_sum(int nPart, const double *partials, const DynGate &g, hipStream_t s, double *dst0, double *dst1 = nullptr, double *dst2 = nullptr) {
    const int col[3] = {0, 1, 2};
    const double scale[3] = {1.0, 1.0, 1.0};
    double *const dst[3] = {dst0, dst1, dst2};
    launch_reduce(nPart, dst2 ? 3 : (dst1 ? 2 : 1), col, scale, dst, partials, g, s);
}

// y = cK y + cM M x (acc) or cM M x; the workgroups' x . y in partials[.][0] (null: not wanted). Returns the number of partials.
int launch_spmv_kron_acc(const SpmvArgs &a, bool acc, double cK, double cM, const double *x, double *y, double *partials, const DynGate &g, hipStream_t s,
                         int cap = DYN_GRID_CAP) {
    if (a.nChunk <= 0) return 0;
    if (a.dim != 2 && a.dim != 3) throw mfh::Error(MFH_ERR_UNSUPPORTED, "k_spmv_kron_acc: 2D / 3D only");
    const size_t lds = ((size_t)a.dim * a.chunkSlots + 16) * sizeof(double);
    const int grid = (int)std::min<int64_t>(a.nChunk, std::max(1, std::min(cap, DYN_GRID_CAP)));
    with_dim(a.dim, [&](auto D) { with_bool(acc, [&](auto ACC) {
        launch_k(k_spmv_kron_acc<D(), ACC()>, dim3(grid), dim3(256), lds, s, a, cK, cM, x, y, partials, g);
    }); });
    CHECK_LAUNCH();
    return grid;
}

void launch_pencil_dinv(int dim, int64_t nRows, const int32_t *rowPtr, const int32_t *colIdx, const double *kVals, const double *mVals, double cK, double cM,
                        const uint8_t *mask, double *dinv, hipStream_t s) {
    with_dim(dim, [&](auto D) { launch_k(k_pencil_dinv<D()>, dim3(grid_for(nRows)), dim3(256), 0, s, nRows, rowPtr, colIdx, kVals, mVals, cK, cM, mask, dinv); });
    CHECK_LAUNCH();
}

}   // namespace
}}   // namespace mfh::k

namespace mfhi { namespace {

using namespace mfh;

// the context conditions of mfh_newmark (those of mfh_modes, but the set of fixed variables may be empty) and the device state both products need
void prepare_pencil(mfh_ctx *c, const char *who) {
    require(c->haveMesh && !c->external, MFH_ERR_STATE, "no mesh set");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    if (!(c->op == MFH_OP_ELASTICITY && c->opDegree != 1))
        throw Error(MFH_ERR_UNSUPPORTED, std::string(who) + ": the operators are (elasticity, mass) on the mesh's own degree: select MFH_OP_ELASTICITY and leave the forced-degree-1 view");
    if (!(!dist_active(c) && c->mesh.nOwned == c->mesh.nNode && c->nOwnedDoF() == c->nDoF)) throw Error(MFH_ERR_UNSUPPORTED, std::string(who) + ": unpartitioned contexts only");
    require(c->mesh.dim == 2 || c->mesh.dim == 3, MFH_ERR_UNSUPPORTED, "2D / 3D meshes");
}

void upload(double *dst, const double *src, int64_t n, hipStream_t s) { MFH_HIP(hipMemcpyAsync(dst, src, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s)); }

// The device state both products read, after prepare_pencil and the caller's WideGuard: K assembled and the fixed-variable mask on the device
// (ensure_precond, which also settles the preconditioner in use: BEFORE the mass buffer), the mass buffer, the lists of the matrix-free operator or
// else both triangles of the assembled one. hierarchy: the levels of the two-level / multigrid preconditioner as well, where that is the one in use
// (for a loop on a context with fixed variables: K's hierarchy needs K definite).
void prepare_pencil_state(mfh_ctx *c, const char *who, bool hierarchy) {
    ensure_precond(c);
    if (hierarchy) ensure_coarse_levels(c, 1);
    ensure_mass(c);
    prepare_matrix_free(c);
    if (!c->use_mf()) require_full_storage(c, ("the assembled SpMV of " + std::string(who)).c_str());
}

// What NewmarkWork (mfh_dynamics.hip) and HarmonicWork (mfh_harmonic.hip) are built on: the sizes, the preconditioner chosen, the buffers of the
// sums, the history {r.z, p.Ap, r.r, -} with its control block, the batch of the next solve and the phase clock. A work adds its vectors (slots
// of vec, ld apart), its coefficients and the launches of its own kernels, and for pencil_loop the members start(jacobi) and iterate(it, jacobi).
struct PencilWork {
    mfh_ctx *c = nullptr;
    hipStream_t s = nullptr;
    int d = 0;
    int64_t n = 0, nRows = 0, ld = 0;  // variables, block rows, n rounded up to 32: the stride of the slots of vec (and of the two planes of a complex vector)
    bool masked = false, wantCoarse = false, useMG = false, useTL = false;     // wantCoarse: the context asks for a hierarchy; useMG / useTL: the loop has one
    const uint8_t *mask = nullptr;
    DBuf<double> vec, partials, scal, ctl, dinv;
    double dinvCK = -1, dinvCM = -1;           // the pencil the inverse diagonal blocks in dinv were built for
    double *stop = nullptr, *bb = nullptr;     // ctl: [0..3] the control block {threshold, -, -, iteration base}, [4] b . b of the right-hand side
    int maxit = 0, batch = 8;
    // per-phase device time (scripts/probe_dynamics.py, scripts/probe_harmonic.py: env MFH_DYN_TIMING=1 puts a synchronisation at every phase boundary)
    bool timing = false;
    double tPhase[7] = {0, 0, 0, 0, 0, 0, 0};  // K products, M products + p.Ap, residual update (+ block-Jacobi), coarse preconditioner + r.z, direction, read-back, step kernels (mfh_newmark)
    double tMark = 0;
    void lap(int phase) {
        if (!timing) return;
        MFH_HIP(hipStreamSynchronize(s));
        const double t = now_ms();
        if (phase >= 0) tPhase[phase] += t - tMark;
        tMark = t;
    }

    k::DynGate gate(int it) const { return k::DynGate{scal.p, it, stop}; }
    void reduce(int nPart, int nv, const int *col, const double *scale, double *const *dst, const k::DynGate &g) { k::launch_reduce(nPart, nv, col, scale, dst, partials.p, g, s); }
    void sum_to(int nPart, const k::DynGate &g, double *dst0, double *dst1 = nullptr, double *dst2 = nullptr) { k::launch_sum(nPart, partials.p, g, s, dst0, dst1, dst2); }
    int vec_grid(int64_t count) const { return k::dyn_grid(count, std::max(1, std::min(c->dynGridCap, k::DYN_GRID_CAP))); }
    int short_batch() const { return std::max(2, std::min(8, c->checkEvery)); }
    // the block-Jacobi of cK K + cM M, rebuilt when the pencil changes
    void ensure_dinv(double cK, double cM) {
        if (dinvCK == cK && dinvCM == cM) return;
        dinv.alloc((size_t)nRows * (size_t)(d * (d + 1) / 2));
        k::launch_pencil_dinv(d, nRows, c->dRowPtr.p, c->dColIdx.p, cK != 0.0 ? c->dVals.p : nullptr, c->dMassVals.p, cK, cM, mask, dinv.p, s);
        dinvCK = cK; dinvCM = cM;
    }
};

// The state of the context the pencil products and the preconditioners read, the base of the work filled in, the choice of the preconditioner (K's
// two-level / multigrid hierarchy where the context asks for one and K is definite on the free variables, the diagonal blocks of the pencil
// otherwise), the buffers of the sums, the history and the control blocks. Returns whether the loop runs block-Jacobi; the caller words its notes
// from (wantCoarse, masked, useMG, useTL), and allocates vec (slots ld apart) and what else its loop keeps.
bool setup_pencil_work(mfh_ctx *c, PencilWork &w, const char *who, int maxit) {
    const bool masked = !c->fixedVars.empty();
    prepare_pencil_state(c, who, masked);
    require(c->sym.nRows == c->sym.nCols, MFH_ERR_UNSUPPORTED, (std::string(who) + ": unpartitioned contexts only").c_str());
    w.c = c; w.s = c->stream; w.d = c->bs();
    w.nRows = c->sym.nRows;
    w.n = (int64_t)w.d * c->nDoF;
    w.ld = (w.n + 31) / 32 * 32;
    w.masked = masked;
    w.mask = masked ? c->dFixedMask.p : nullptr;
    w.maxit = maxit;
    w.wantCoarse = c->precond == MFH_PRECOND_TWO_LEVEL || c->precond == MFH_PRECOND_MULTIGRID;
    w.useMG = masked && c->precond == MFH_PRECOND_MULTIGRID && c->mg.valid && !c->mg.singular;
    w.useTL = masked && !w.useMG && w.wantCoarse && c->tl.valid;
    w.partials.alloc((size_t)k::DYN_GRID_CAP * k::DYN_NV);
    w.scal.alloc(((size_t)maxit + 2) * 4);
    w.ctl.alloc(8);
    w.ctl.zero(w.s);
    w.stop = w.ctl.p; w.bb = w.ctl.p + 4;
    c->stop.alloc(4);                  // (the control block tl_precond hands its kernel; not read without a history)
    c->stop.zero(w.s);
    w.batch = w.short_batch();
    w.timing = getenv("MFH_DYN_TIMING") != nullptr;
    return !(w.useMG || w.useTL);
}

// The host side of one solve, for both loops: w.start(jacobi) forms the first residual and direction, then batches of w.iterate(it, jacobi); after
// each batch the history since the last check and the control block come back (the one synchronisation) and are scanned. Returns the first q with
// r.r of iterate q <= the threshold (the gate has made the kernels of later iterations no-ops: x is iterate q), -1: maxit reached (x then holds the
// last iterate), -2: breakdown (a residual norm is not finite). first: iterations before the first check; later(): before each further one;
// remember: a solve that converged at q leaves w.batch = q + 1 (within [2, check_every]) for the next -- it needs about as many: one read-back.
template <class Work, class Later>
int pencil_loop(Work &w, bool jacobi, int first, Later &&later, bool remember) {
    MFH_HIP(hipMemsetAsync(w.scal.p, 0, w.scal.n * sizeof(double), w.s));
    w.start(jacobi);
    std::vector<double> hs;
    double hctl[5];
    int it = 0, lastChecked = 0, step = first;
    for (;;) {
        const int itEnd = std::min(w.maxit, it + step);
        for (; it < itEnd; ++it) w.iterate(it, jacobi);
        hs.resize((size_t)(it - lastChecked + 1) * 4);
        MFH_HIP(hipMemcpyAsync(hs.data(), w.scal.p + (size_t)lastChecked * 4, hs.size() * sizeof(double), hipMemcpyDeviceToHost, w.s));
        MFH_HIP(hipMemcpyAsync(hctl, w.ctl.p, sizeof(hctl), hipMemcpyDeviceToHost, w.s));
        MFH_HIP(hipStreamSynchronize(w.s));
        w.lap(5);
        for (int q = lastChecked; q <= it; ++q) {
            const double rr = hs[(size_t)(q - lastChecked) * 4 + 2];
            if (!std::isfinite(rr)) return -2;
            if (rr <= hctl[0]) {
                if (remember) w.batch = std::max(2, std::min(q + 1, w.c->checkEvery));
                return q;
            }
        }
        if (it >= w.maxit) return -1;
        lastChecked = it;
        step = later();
    }
}

}}   // namespace mfhi
