// Explicit dynamics (mfh_mass_lumped_hrz, mfh_explicit_dt, mfh_explicit, include/meshfem_hip.h; docs/design/04_20_explicit_dynamics.md): central
// differences in velocity-Verlet form on
//   M_L u'' + aR M_L u' + K u = g(t) f,   M_L = density x the HRZ-lumped mass matrix (a positive diagonal on every element type),
// fixed variables held at zero by a zero in the inverse-mass vector. The reference has no time integrator; the scheme is checked against an
// independent recurrence (tests/explicit_util.py). Only the K product of the context is used (apply_operator): no mass buffer, no widened
// pattern, no hierarchy.
//   k_mass_hrz          m_d = sum over the pairs (e, i) of DoF d of rho_e vol_e w_i, w_i = Mref_ii / trace(Mref); gather over the DoF-pair list
//   k_explicit_masses   density m and its inverse (0 on the fixed variables) per variable
//   k_gersh_gather      g = (sum over the pairs of the element's absolute row sums, k_elem_abs_rowsums of mfh_kernels.hip) / m, the workgroup's
//                       maximum over the free variables; k_max_finish takes the maximum of those
//   k_power_default_start  the documented default start vector;
//   k_power_start       x . M x of the start vector;  k_power_step: one step x <- M^-1 K x of the power iteration behind the K product
//   k_explicit_step     the kick of step n and the drift of step n + 1, probes, snapshot row, energy partials, the non-finite flag
// No floating-point atomics: a lane adds its pairs in list order, sums go through one partial per workgroup and k_dyn_reduce (mfh_pencil.hh), the
// grids depend on n and option dyn_grid_cap only -- the same call returns the same bits.
#include "mfh_pencil.hh"
#include <cfloat>

namespace mfh { namespace k {

namespace {

constexpr int npe_of(int dim, int deg) { return dim == 3 ? (deg == 1 ? 4 : 10) : (deg == 1 ? 3 : 6); }

struct HrzArgs {
    int64_t nDoF;
    int geoStride;
    const int32_t *dofPtr, *dofPair;
    const double *geo;
    double w[10];                // HRZ weights of the local nodes
};

// one lane per DoF, the pairs of a DoF added in list order; the value is repeated for the DIM components
template <int DIM, int DEG>
__global__ void __launch_bounds__(256) k_mass_hrz(HrzArgs a, const double *__restrict__ density, double *__restrict__ out) {
    constexpr int NPE = npe_of(DIM, DEG);
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < a.nDoF; r += (int64_t)gridDim.x * 256) {
        double acc = 0.0;
        const int last = a.dofPtr[r + 1];
        for (int q = a.dofPtr[r]; q < last; ++q) {
            const int64_t code = a.dofPair[q], e = code / NPE;
            const int i = (int)(code - e * NPE);
            const double vol = a.geo[e * a.geoStride + 12];
            const double rv = density ? density[e] * vol : vol;
            // runtime-indexed kernel-argument array: read through a select chain over the small table
            double wi = 0;
#pragma unroll
            for (int k = 0; k < NPE; ++k) wi = (k == i) ? a.w[k] : wi;
            acc += rv * wi;
        }
#pragma unroll
        for (int c = 0; c < DIM; ++c) out[r * DIM + c] = acc;
    }
}

// mass = density m, inv = 1 / mass, 0 on the fixed variables
__global__ void __launch_bounds__(256) k_explicit_masses(int64_t n, double density, const double *__restrict__ m, const uint8_t *__restrict__ mask,
                                                        double *__restrict__ mass, double *__restrict__ inv) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = density * m[i];
        mass[i] = v;
        inv[i] = (mask && mask[i]) ? 0.0 : 1.0 / v;
    }
}

DEV double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    return v;
}
// block-wide maximum, valid in thread 0; lds: 4 doubles
DEV double block_max(double v, double *lds) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) v = fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
    __syncthreads();
    return v;
}

// rs: [nElem][NPE][DIM] absolute row sums; m: [nDoF][DIM] lumped masses; partMax[blockIdx.x] = max over the workgroup's free variables of g
template <int DIM, int DEG>
__global__ void __launch_bounds__(256) k_gersh_gather(int64_t nDoF, const int32_t *__restrict__ dofPtr, const int32_t *__restrict__ dofPair,
                                                     const double *__restrict__ rs, const double *__restrict__ m, const uint8_t *__restrict__ mask,
                                                     double *__restrict__ partMax) {
    __shared__ double red[4];
    double best = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nDoF; r += (int64_t)gridDim.x * 256) {
        double acc[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
        const int last = dofPtr[r + 1];
        for (int q = dofPtr[r]; q < last; ++q) {
            const int64_t code = dofPair[q];
#pragma unroll
            for (int c = 0; c < DIM; ++c) acc[c] += rs[code * DIM + c];
        }
#pragma unroll
        for (int c = 0; c < DIM; ++c)
            if (!(mask && mask[r * DIM + c])) best = fmax(best, acc[c] / m[r * DIM + c]);
    }
    best = block_max(best, red);
    if (threadIdx.x == 0) partMax[blockIdx.x] = best;
}

__global__ void __launch_bounds__(256) k_max_finish(int nPart, const double *__restrict__ partMax, double *__restrict__ out) {
    __shared__ double red[4];
    double best = 0.0;
    for (int b = threadIdx.x; b < nPart; b += 256) best = fmax(best, partMax[b]);
    best = block_max(best, red);
    if (threadIdx.x == 0) out[0] = best;
}

// the default start vector of the power iteration: a fixed hash of the variable index, in [-1/2, 1/2) -- integer arithmetic and one exact scaling, so
// the host (a test's restatement) and the device form the same bits
__host__ __device__ inline double power_default_start(int64_t i) {
    return (double)((uint32_t)((uint64_t)(i + 1) * 2654435761ull) >> 8) * (1.0 / 16777216.0) - 0.5;
}
__global__ void __launch_bounds__(256) k_power_default_start(int64_t n, double *__restrict__ x) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] = power_default_start(i);
}

// x = 0 on the fixed variables; partials[.][0] = x . mass x
__global__ void __launch_bounds__(256) k_power_start(int64_t n, const double *__restrict__ mass, const uint8_t *__restrict__ mask, double *__restrict__ x,
                                                    double *__restrict__ partials) {
    __shared__ double red[4];
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double xi = x[i];
        if (mask && mask[i]) { xi = 0.0; x[i] = 0.0; }
        acc[0] = fma(mass[i] * xi, xi, acc[0]);
    }
    store_partials<1>(acc, red, partials);
}

// With s = 1 / sqrt(nrm[0]) (nrm = x . M x of the vector in x, left by the previous step's second stage), xn = s x, yn = s y (y = K x):
//   partials[.][0] = xn . yn   (the Rayleigh quotient of xn, which has unit M-norm),   x <- z = inv yn,   partials[.][1] = z . yn = z . M z
__global__ void __launch_bounds__(256) k_power_step(int64_t n, const double *__restrict__ y, const double *__restrict__ inv, const double *__restrict__ nrm,
                                                   double *__restrict__ x, double *__restrict__ partials) {
    __shared__ double red[8];
    const double s = 1.0 / sqrt(nrm[0]);
    double acc[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double yn = s * y[i], xn = s * x[i];
        const double z = inv[i] * yn;
        x[i] = z;
        acc[0] = fma(xn, yn, acc[0]);
        acc[1] = fma(z, yn, acc[1]);
    }
    store_partials<2>(acc, red, partials);
}

// ---- the step kernel
struct StepArgs {
    int64_t n;
    double dt, hdt, alpha, den;   // hdt = dt / 2, den = 1 + alpha dt / 2
    int mode;                    // 0: v holds v(n - 1/2); 1: the first step, v holds v0 and a0 = inv (g f - y) - alpha v0; 2: the first step, a0 is read from a
    int last;                    // 1: a(n) and v(n) are written to a and v, u stays (no drift)
    int step;                    // n: amplitude[n] is g (amplitude null: 1)
    int wantEnergy;              // the workgroup's partials of the four sums are stored
    int nProbe;
    const double *amplitude;
    const int64_t *probeVars;
    double *probeRow;            // nProbe values of this step (null: no probes)
    double *snapRow;             // n values (null: not a snapshot step)
    int *flag;                   // set to 1 by every lane that meets a value that is not finite
};

// one variable: the kick of step n (a, v at n from y = K u(n)) and the drift to n + 1. Every product-sum is an explicit fma, so that a run cut in
// two (state handed over through memory) rounds as the uncut run does.
DEV void explicit_point(const StepArgs &p, double g, double y, double uk, double vin, double im, double fi, double ain, double mi, double (&acc)[4],
                        double &un, double &vh, double &ak, double &vk) {
    if (p.mode == 0) {
        const double t = im * fma(g, fi, -y);
        ak = fma(-p.alpha, vin, t) / p.den;
        vk = fma(p.hdt, ak, vin);
    } else {
        vk = vin;
        ak = p.mode == 2 ? ain : fma(-p.alpha, vin, im * fma(g, fi, -y));
    }
    vh = fma(p.hdt, ak, vk);
    un = fma(p.dt, vh, uk);
    if (p.wantEnergy) {
        acc[0] = fma(mi * vk, vk, acc[0]);
        acc[1] = fma(uk, y, acc[1]);
        acc[2] = fma(g * fi, uk, acc[2]);
        acc[3] = fma(mi * vh, vh, fma(un, y, acc[3]));
    }
}
DEV bool not_finite(double x) { return !(fabs(x) <= DBL_MAX); }

// Reads y, uIn, v, inv, f (and a in mode 2, mass on energy steps); writes uOut and v (on the last step: a and v). uIn and uOut are two buffers
// the host swaps, so that the probes may read uIn from any lane. The lanes take two consecutive variables (16-byte accesses: every vector starts on
// a 256-byte boundary); the last variable of an odd n is taken alone.
__global__ void __launch_bounds__(256) k_explicit_step(StepArgs p, const double *__restrict__ y, const double *__restrict__ uIn, double *__restrict__ uOut,
                                                      double *__restrict__ v, const double *__restrict__ inv, const double *__restrict__ f,
                                                      double *__restrict__ a, const double *__restrict__ mass, double *__restrict__ partials) {
    __shared__ double red[16];
    const double g = p.amplitude ? p.amplitude[p.step] : 1.0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < p.nProbe; j += (int64_t)gridDim.x * 256) p.probeRow[j] = uIn[p.probeVars[j]];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    bool bad = false;
    const int64_t nPair = p.n >> 1;
    const bool snapVec = p.snapRow && (reinterpret_cast<uintptr_t>(p.snapRow) & 15) == 0;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nPair; q += (int64_t)gridDim.x * 256) {
        const double2 y2 = reinterpret_cast<const double2 *>(y)[q], u2 = reinterpret_cast<const double2 *>(uIn)[q];
        const double2 v2 = reinterpret_cast<const double2 *>(v)[q], i2 = reinterpret_cast<const double2 *>(inv)[q];
        double2 f2 = {0.0, 0.0}, a2 = {0.0, 0.0}, m2 = {0.0, 0.0};
        if (f) f2 = reinterpret_cast<const double2 *>(f)[q];
        if (p.mode == 2) a2 = reinterpret_cast<const double2 *>(a)[q];
        if (p.wantEnergy) m2 = reinterpret_cast<const double2 *>(mass)[q];
        double2 un, vh, ak, vk;
        explicit_point(p, g, y2.x, u2.x, v2.x, i2.x, f2.x, a2.x, m2.x, acc, un.x, vh.x, ak.x, vk.x);
        explicit_point(p, g, y2.y, u2.y, v2.y, i2.y, f2.y, a2.y, m2.y, acc, un.y, vh.y, ak.y, vk.y);
        if (p.snapRow) {
            if (snapVec) reinterpret_cast<double2 *>(p.snapRow)[q] = u2;
            else { p.snapRow[2 * q] = u2.x; p.snapRow[2 * q + 1] = u2.y; }
        }
        if (p.last) {
            reinterpret_cast<double2 *>(a)[q] = ak;
            reinterpret_cast<double2 *>(v)[q] = vk;
            bad = bad || not_finite(ak.x) || not_finite(ak.y) || not_finite(vk.x) || not_finite(vk.y);
        } else {
            reinterpret_cast<double2 *>(uOut)[q] = un;
            reinterpret_cast<double2 *>(v)[q] = vh;
            bad = bad || not_finite(un.x) || not_finite(un.y) || not_finite(vh.x) || not_finite(vh.y);
        }
    }
    if ((p.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = p.n - 1;
        const double uk = uIn[i];
        double un, vh, ak, vk;
        explicit_point(p, g, y[i], uk, v[i], inv[i], f ? f[i] : 0.0, p.mode == 2 ? a[i] : 0.0, p.wantEnergy ? mass[i] : 0.0, acc, un, vh, ak, vk);
        if (p.snapRow) p.snapRow[i] = uk;
        if (p.last) { a[i] = ak; v[i] = vk; bad = bad || not_finite(ak) || not_finite(vk); }
        else { uOut[i] = un; v[i] = vh; bad = bad || not_finite(un) || not_finite(vh); }
    }
    if (bad) p.flag[0] = 1;
    if (p.wantEnergy) store_partials<4>(acc, red, partials);     // (uniform)
}

int launch_explicit_step(const StepArgs &p, const double *y, const double *uIn, double *uOut, double *v, const double *inv, const double *f, double *a,
                         const double *mass, double *partials, int cap, hipStream_t s) {
    const int grid = dyn_grid(std::max<int64_t>(p.n >> 1, 1), std::max(1, std::min(cap, DYN_GRID_CAP)));
    hipLaunchKernelGGL(k_explicit_step, dim3(grid), dim3(256), 0, s, p, y, uIn, uOut, v, inv, f, a, mass, partials);
    CHECK_LAUNCH();
    return grid;
}

}   // namespace
}}   // namespace mfh::k

using namespace mfh;
using namespace mfhi;

namespace {

constexpr int EXP_BATCH = 256;           // steps between two reads of the non-finite flag (the one synchronisation of a batch)

// the HRZ weights of the element type from the mass quadrature table (ShapeTables::massRef): Mref_ii / trace(Mref)
// (trace and quotient in long double, rounded once: a weight multiplies every pair of a DoF, so its error is not averaged out by the sum)
void hrz_weights(const ShapeTables &T, int npe, double *w) {
    long double tr = 0.0L;
    for (int i = 0; i < npe; ++i) tr += (long double)T.massRef[(size_t)i * npe + i];
    for (int i = 0; i < npe; ++i) w[i] = (double)((long double)T.massRef[(size_t)i * npe + i] / tr);
}

// out[dim nDoF] (device) = the HRZ-lumped masses under the context's density field
void launch_mass_hrz(mfh_ctx *c, double *out) {
    ensure_geometry(c);
    ensure_dof_pairs(c);
    const HostMesh &m = c->mesh;
    k::HrzArgs a{};
    a.nDoF = c->nDoF; a.geoStride = c->geoStride; a.dofPtr = dof_pair_ptr(c); a.dofPair = dof_pair_list(c); a.geo = c->dGeo.p;
    hrz_weights(c->tables, m.npe, a.w);
    const int grid = k::grid_for(c->nDoF, std::max(1, std::min(c->dynGridCap, k::DYN_GRID_CAP)));
    const double *rho = c->haveDensity ? c->dDensity.p : nullptr;
    k::with_dim_deg(m.dim, m.deg, [&](auto D, auto G) { k::launch_k(k::k_mass_hrz<D(), G()>, dim3(grid), dim3(256), 0, c->stream, a, rho, out); });
    CHECK_LAUNCH();
}

// What mfh_explicit_dt and mfh_explicit share: the device state the K product reads (K assembled where the operator is the assembled one, the
// fixed-variable mask, the lists of the matrix-free operator) and the vectors: density M_L, its masked inverse, the work slots.
struct ExplicitWork {
    mfh_ctx *c = nullptr;
    hipStream_t s = nullptr;
    int d = 0, cap = 1;
    int64_t n = 0, ld = 0;
    bool masked = false;
    const uint8_t *mask = nullptr;
    DBuf<double> vec, partials, scal;
    double *mass = nullptr, *inv = nullptr, *y = nullptr, *x = nullptr;      // slots 0 .. 3; the stepper adds its own behind them
    int grid(int64_t count) const { return k::dyn_grid(count, cap); }
};

void setup_explicit_work(mfh_ctx *c, ExplicitWork &w, double density, int slots) {
    // K as the operator reads it and the fixed-variable mask on the device; no preconditioner is set up (ensure_precond would extract the inverse
    // diagonal blocks). Its one refusal that concerns the K product is repeated here.
    ensure_assembled(c);
    ensure_fixed_uploaded(c);
    prepare_matrix_free(c);
    if (c->deterministic && c->use_mf() && c->mfModeEff() != 4)
        throw Error(MFH_ERR_UNSUPPORTED, "option deterministic: the matrix-free operator must be the cluster variant (matrix_free_mode 4) or the assembled SpMV (matrix_free 0)");
    w.c = c; w.s = c->stream; w.d = c->bs();
    w.cap = std::max(1, std::min(c->dynGridCap, k::DYN_GRID_CAP));
    w.n = (int64_t)w.d * c->nDoF;
    w.ld = (w.n + 31) / 32 * 32;
    w.masked = !c->fixedVars.empty();
    w.mask = w.masked ? c->dFixedMask.p : nullptr;
    w.vec.alloc((size_t)w.ld * (size_t)slots);
    w.vec.zero(w.s);
    w.partials.alloc((size_t)k::DYN_GRID_CAP * k::DYN_NV);
    w.scal.alloc(8);
    w.scal.zero(w.s);
    w.mass = w.vec.p; w.inv = w.mass + w.ld; w.y = w.inv + w.ld; w.x = w.y + w.ld;
    launch_mass_hrz(c, w.y);
    hipLaunchKernelGGL(k::k_explicit_masses, dim3(w.grid(w.n)), dim3(256), 0, w.s, w.n, density, (const double *)w.y, w.mask, w.mass, w.inv);
    CHECK_LAUNCH();
}

// iters steps of x <- M^-1 K x on the free variables from x0 (null: the default start vector); returns the last Rayleigh quotient
double power_iteration(ExplicitWork &w, int iters, const double *x0) {
    mfh_ctx *c = w.c;
    hipStream_t s = w.s;
    double *nrm = w.scal.p, *lam = w.scal.p + 1;
    const int g0 = w.grid(w.n);
    if (x0) upload(w.x, x0, w.n, s);
    else {
        hipLaunchKernelGGL(k::k_power_default_start, dim3(g0), dim3(256), 0, s, w.n, w.x);
        CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k::k_power_start, dim3(g0), dim3(256), 0, s, w.n, (const double *)w.mass, w.mask, w.x, w.partials.p);
    CHECK_LAUNCH();
    k::launch_sum(g0, w.partials.p, k::dyn_open(), s, nrm);
    for (int it = 0; it < iters; ++it) {
        apply_operator(c, w.masked, w.x, w.y, nullptr);
        hipLaunchKernelGGL(k::k_power_step, dim3(g0), dim3(256), 0, s, w.n, (const double *)w.y, (const double *)w.inv, (const double *)nrm, w.x, w.partials.p);
        CHECK_LAUNCH();
        k::launch_sum(g0, w.partials.p, k::dyn_open(), s, lam, nrm);
    }
    double out = 0.0;
    MFH_HIP(hipMemcpyAsync(&out, lam, sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    return out;
}

void check_explicit_params(const mfh_explicit_params *p) {
    require(p != nullptr, MFH_ERR_INVALID, "mfh_explicit: params is null");
    require(p->dt > 0.0 && std::isfinite(p->dt), MFH_ERR_INVALID, "mfh_explicit: dt > 0");
    require(p->density > 0.0 && std::isfinite(p->density), MFH_ERR_INVALID, "mfh_explicit: density > 0");
    require(p->rayleighMass >= 0.0 && std::isfinite(p->rayleighMass), MFH_ERR_INVALID, "mfh_explicit: the mass-proportional damping coefficient is not negative");
    require(p->nSteps >= 0 && p->snapshotStride >= 0 && p->energyStride >= 0, MFH_ERR_INVALID, "mfh_explicit: nSteps >= 0, snapshotStride >= 0, energyStride >= 0");
    require((p->flags & ~(MFH_EXP_HAVE_ACCEL | MFH_EXP_ENERGIES | MFH_EXP_NO_DT_CHECK)) == 0, MFH_ERR_INVALID, "mfh_explicit: unknown flag");
}

}   // namespace

extern "C" {

mfh_status mfh_mass_lumped_hrz(mfh_ctx *c, double *diagOut, int32_t flags) {
    MFH_TRY(c)
    require(c && diagOut, MFH_ERR_INVALID, "mfh_mass_lumped_hrz: null argument");
    require((flags & ~MFH_LOAD_ON_DEVICE) == 0, MFH_ERR_INVALID, "flags: 0 | MFH_LOAD_ON_DEVICE");
    require(c->haveMesh && !c->hostOnly && !c->external, MFH_ERR_STATE, "the lumped mass matrix needs a mesh on a device");
    prepare_pencil(c, "mfh_mass_lumped_hrz");
    const size_t n = (size_t)c->mesh.dim * (size_t)c->nDoF;
    DBuf<double> tmp;
    double *out = diagOut;
    if (!(flags & MFH_LOAD_ON_DEVICE)) { tmp.alloc(n); out = tmp.p; }
    launch_mass_hrz(c, out);
    if (!(flags & MFH_LOAD_ON_DEVICE)) tmp.download(diagOut, n, c->stream);
    else MFH_HIP(hipStreamSynchronize(c->stream));
    MFH_CATCH(c)
}

mfh_status mfh_explicit_dt(mfh_ctx *c, double density, int32_t iters, const double *x0, mfh_explicit_dt_info *info) {
    if (info) { *info = mfh_explicit_dt_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c && info, MFH_ERR_INVALID, "mfh_explicit_dt: null argument");
    require(density > 0.0 && std::isfinite(density), MFH_ERR_INVALID, "mfh_explicit_dt: density > 0");
    require(iters >= 0, MFH_ERR_INVALID, "mfh_explicit_dt: iters >= 0 (0: 60)");
    prepare_pencil(c, "mfh_explicit_dt");
    hipStream_t s = c->stream;
    c->dynNote.clear();
    EventTimer t(s);
    ExplicitWork w;
    setup_explicit_work(c, w, density, 4);
    // the guaranteed bound: Gershgorin on M_L^-1 K with the triangle inequality over the elements of a row
    const HostMesh &m = c->mesh;
    DBuf<double> rs, pmax;
    rs.alloc((size_t)m.nElem * (size_t)m.npe * (size_t)m.dim);
    k::launch_elem_abs_rowsums(asm_args(c), rs.p, 4 * w.cap, s);
    const int grid = k::grid_for(c->nDoF, w.cap);
    pmax.alloc((size_t)grid + 1);
    k::with_dim_deg(m.dim, m.deg, [&](auto D, auto G) {
        k::launch_k(k::k_gersh_gather<D(), G()>, dim3(grid), dim3(256), 0, s, c->nDoF, dof_pair_ptr(c), dof_pair_list(c), (const double *)rs.p, (const double *)w.mass,
                    w.mask, pmax.p);
    });
    CHECK_LAUNCH();
    hipLaunchKernelGGL(k::k_max_finish, dim3(1), dim3(256), 0, s, grid, (const double *)pmax.p, pmax.p + grid);
    CHECK_LAUNCH();
    double upper = 0.0;
    MFH_HIP(hipMemcpyAsync(&upper, pmax.p + grid, sizeof(double), hipMemcpyDeviceToHost, s));
    const int its = iters == 0 ? 60 : iters;
    const double est = power_iteration(w, its, x0);            // (synchronises)
    info->lambdaUpper = upper;
    info->lambdaEst = est;
    info->dtSafe = 2.0 / std::sqrt(upper);
    info->dtEst = 2.0 / std::sqrt(est);
    info->iterations = its;
    info->ms = t.stop();
    if (!(est > 0.0) || !std::isfinite(est)) {
        c->dynNote = "the power iteration found no positive Rayleigh quotient (a start vector without a free component, or K x = 0)";
        info->note = c->dynNote.c_str();
        throw Error(MFH_ERR_INVALID, "mfh_explicit_dt: " + c->dynNote);
    }
    info->note = c->dynNote.c_str();
    MFH_CATCH(c)
}

mfh_status mfh_explicit(mfh_ctx *c, const mfh_explicit_params *prm, double *u, double *v, double *a, const double *f, const double *amplitude,
                        const int64_t *probeVars, int32_t nProbe, double *probeOut, double *snapshots, double *energies, mfh_explicit_info *info) {
    if (info) { *info = mfh_explicit_info{}; info->note = ""; }
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_explicit: null context");
    check_explicit_params(prm);
    const mfh_explicit_params P = *prm;
    require(u && v && a, MFH_ERR_INVALID, "mfh_explicit: u, v and a are not null");
    require(nProbe >= 0 && (nProbe == 0 || (probeVars && probeOut)), MFH_ERR_INVALID, "mfh_explicit: probes need their variables and their output");
    const bool wantE = (P.flags & MFH_EXP_ENERGIES) != 0;
    require(!energies || wantE, MFH_ERR_INVALID, "mfh_explicit: energies given without MFH_EXP_ENERGIES");
    require(!wantE || energies, MFH_ERR_INVALID, "mfh_explicit: MFH_EXP_ENERGIES needs the energies array");
    require(!snapshots || P.snapshotStride > 0, MFH_ERR_INVALID, "mfh_explicit: snapshots need snapshotStride > 0");
    if (c->haveMesh && !c->external) {
        const int64_t nv = (int64_t)c->bs() * c->nDoF;
        for (int32_t j = 0; j < nProbe; ++j) require(probeVars[j] >= 0 && probeVars[j] < nv, MFH_ERR_INVALID, "mfh_explicit: probe variable out of range");
    }
    prepare_pencil(c, "mfh_explicit");
    hipStream_t s = c->stream;
    c->dynNote.clear();
    EventTimer tsetup(s);
    ExplicitWork w;
    setup_explicit_work(c, w, P.density, 8);
    double *ub[2] = {w.x, w.x + w.ld};
    double *vh = w.x + 2 * w.ld, *acc = w.x + 3 * w.ld, *fv = w.x + 4 * w.ld;      // (slot 3 = x serves the power iteration first, then u)

    // ---- step-size policy: lambdaEst is a lower bound of lambda_max, so dt > 2 / sqrt(lambdaEst) is certainly unstable
    if (!(P.flags & MFH_EXP_NO_DT_CHECK)) {
        const double est = power_iteration(w, 60, nullptr);
        // (what mfh_explicit_dt refuses: no free variable, or K x = 0 for the start vector -- there is no estimate to check dt against)
        if (!(est > 0.0) || !std::isfinite(est))
            throw Error(MFH_ERR_INVALID, "mfh_explicit: the power iteration found no positive Rayleigh quotient (no free variable, or K x = 0 for the start vector): no estimate of the "
                                         "stability limit to check dt against (MFH_EXP_NO_DT_CHECK runs without one)");
        if (info) { info->lambdaEst = est; info->dtEst = 2.0 / std::sqrt(est); }
        if (P.dt > 2.0 / std::sqrt(est))
            throw Error(MFH_ERR_INVALID, "mfh_explicit: dt = " + std::to_string(P.dt) + " exceeds the stability limit 2 / sqrt(lambda_max) <= " + std::to_string(2.0 / std::sqrt(est)) +
                                             " (mfh_explicit_dt; MFH_EXP_NO_DT_CHECK runs it all the same)");
    }

    const int nSteps = P.nSteps;
    const int stride = snapshots ? P.snapshotStride : 0;
    const int eStride = wantE ? std::max(1, P.energyStride) : 0;
    const int64_t nSnapRows = stride ? nSteps / stride + 1 : 0;
    // snapshot rows wait on the device and leave in groups (256 MB at most, one row at least)
    const int64_t snapCap = stride ? std::max<int64_t>(1, std::min<int64_t>(nSnapRows, ((int64_t)1 << 25) / std::max<int64_t>(w.n, 1))) : 0;
    DBuf<double> dSnap, dProbe, dEnergy, dAmp;
    DBuf<int64_t> dProbeVars;
    DBuf<int> dFlag;
    dFlag.alloc(1);
    dFlag.zero(s);
    if (stride) dSnap.alloc((size_t)snapCap * (size_t)w.n);
    if (nProbe) {
        dProbe.alloc((size_t)(nSteps + 1) * (size_t)nProbe);
        dProbeVars.alloc((size_t)nProbe);
        MFH_HIP(hipMemcpyAsync(dProbeVars.p, probeVars, (size_t)nProbe * sizeof(int64_t), hipMemcpyHostToDevice, s));
    }
    if (wantE) { dEnergy.alloc((size_t)(nSteps / eStride + 1) * 4); dEnergy.zero(s); }
    if (amplitude) { dAmp.alloc((size_t)nSteps + 1); upload(dAmp.p, amplitude, (int64_t)nSteps + 1, s); }
    upload(ub[0], u, w.n, s);
    upload(vh, v, w.n, s);
    if (P.flags & MFH_EXP_HAVE_ACCEL) upload(acc, a, w.n, s);
    if (f) upload(fv, f, w.n, s);
    if (w.masked) { k::launch_mask(w.n, w.mask, ub[0], s); k::launch_mask(w.n, w.mask, vh, s); k::launch_mask(w.n, w.mask, acc, s); }
    MFH_HIP(hipStreamSynchronize(s));
    const double setupMs = tsetup.stop();

    EventTimer tsolve(s);
    int64_t snapHeld = 0, snapWritten = 0;
    auto flush_snapshots = [&]() {
        if (snapHeld) MFH_HIP(hipMemcpyAsync(snapshots + (size_t)snapWritten * (size_t)w.n, dSnap.p, (size_t)snapHeld * (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
        MFH_HIP(hipStreamSynchronize(s));
        snapWritten += snapHeld;
        snapHeld = 0;
    };
    k::StepArgs sa{};
    sa.n = w.n; sa.dt = P.dt; sa.hdt = 0.5 * P.dt; sa.alpha = P.rayleighMass; sa.den = 1.0 + P.rayleighMass * (0.5 * P.dt);
    sa.nProbe = nProbe; sa.amplitude = dAmp.p; sa.probeVars = dProbeVars.p; sa.flag = dFlag.p;
    int cur = 0, stepsDone = -1, lastClean = -1;
    bool blewUp = false;
    for (int step = 0; step <= nSteps; ++step) {
        apply_operator(c, w.masked, ub[cur], w.y, nullptr);
        sa.mode = step > 0 ? 0 : ((P.flags & MFH_EXP_HAVE_ACCEL) ? 2 : 1);
        sa.last = step == nSteps;
        sa.step = step;
        sa.wantEnergy = eStride && step % eStride == 0;
        sa.probeRow = nProbe ? dProbe.p + (size_t)step * (size_t)nProbe : nullptr;
        sa.snapRow = nullptr;
        if (stride && step % stride == 0) {
            if (snapHeld == snapCap) flush_snapshots();
            sa.snapRow = dSnap.p + (size_t)snapHeld * (size_t)w.n;
            ++snapHeld;
        }
        const int np = k::launch_explicit_step(sa, w.y, ub[cur], ub[1 - cur], vh, w.inv, f ? fv : nullptr, acc, w.mass, w.partials.p, w.cap, s);
        if (sa.wantEnergy) {
            double *row = dEnergy.p + (size_t)(step / eStride) * 4;
            const int col[4] = {0, 1, 2, 3};
            const double sc[4] = {0.5, 0.5, 1.0, 0.5};
            double *const dst[4] = {row, row + 1, row + 2, row + 3};
            k::launch_reduce(np, 4, col, sc, dst, w.partials.p, k::dyn_open(), s);
        }
        if (!sa.last) cur = 1 - cur;
        if (sa.last || (step + 1) % EXP_BATCH == 0) {            // a batch boundary: the one read of the flag
            int h = 0;
            MFH_HIP(hipMemcpyAsync(&h, dFlag.p, sizeof(int), hipMemcpyDeviceToHost, s));
            MFH_HIP(hipStreamSynchronize(s));
            if (h) { blewUp = true; break; }
            lastClean = step;
        }
    }
    stepsDone = blewUp ? std::max(lastClean, 0) : nSteps;
    if (stride) {
        if (blewUp) { MFH_HIP(hipStreamSynchronize(s)); snapHeld = 0; }     // (rows of the failed batch are not delivered)
        else flush_snapshots();
    }
    if (!blewUp) {
        MFH_HIP(hipMemcpyAsync(u, ub[cur], (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
        MFH_HIP(hipMemcpyAsync(v, vh, (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
        MFH_HIP(hipMemcpyAsync(a, acc, (size_t)w.n * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    {
        const size_t rows = (size_t)(blewUp ? lastClean + 1 : nSteps + 1);
        if (nProbe && rows) MFH_HIP(hipMemcpyAsync(probeOut, dProbe.p, rows * (size_t)nProbe * sizeof(double), hipMemcpyDeviceToHost, s));
        const size_t erows = wantE ? (blewUp ? (size_t)(lastClean >= 0 ? lastClean / eStride + 1 : 0) : (size_t)(nSteps / eStride + 1)) : 0;
        if (erows) MFH_HIP(hipMemcpyAsync(energies, dEnergy.p, erows * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    MFH_HIP(hipStreamSynchronize(s));
    const double solveMs = tsolve.stop();
    if (info) {
        info->stepsDone = stepsDone;
        info->solve_ms = solveMs; info->setup_ms = setupMs;
        info->note = c->dynNote.c_str();
    }
    if (blewUp)
        throw Error(MFH_ERR_NOT_CONVERGED, "mfh_explicit: a value that is not finite appeared after step " + std::to_string(stepsDone) +
                                               " (the time step exceeds the stability limit: mfh_explicit_dt); u, v and a are left as they were passed");
    MFH_CATCH(c)
}

// ---- test hooks (include/meshfem_hip_extras.h)
// k_explicit_step on host arrays of n doubles under the context's dyn_grid_cap. u: u(n) in, u(n + 1) out (last: unchanged); v: v(n - 1/2) (mode 0) or
// v(n) (modes 1, 2) in, v(n + 1/2) (last: v(n)) out; a: read in mode 2, written when last. energies: 4 values or NULL; flag: 1 if a value is not finite.
mfh_status mfh_debug_explicit_step(mfh_ctx *c, int64_t n, double dt, double alpha, double g, int32_t mode, int32_t last, const double *y, double *u, double *v,
                                   const double *inv, const double *mass, const double *f, double *a, const int64_t *probeVars, int32_t nProbe,
                                   double *probeOut, double *snapshot, double *energies, int32_t *flag) {
    MFH_TRY(c)
    require(c && n >= 1 && y && u && v && inv && a && flag && dt > 0 && alpha >= 0 && mode >= 0 && mode <= 2 && nProbe >= 0 && (nProbe == 0 || (probeVars && probeOut)) &&
                (!energies || mass), MFH_ERR_INVALID, "mfh_debug_explicit_step: arguments");
    for (int32_t j = 0; j < nProbe; ++j) require(probeVars[j] >= 0 && probeVars[j] < n, MFH_ERR_INVALID, "mfh_debug_explicit_step: probe variable out of range");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t ld = (n + 31) / 32 * 32;
    DBuf<double> buf, part, amp;
    DBuf<int64_t> dv;
    DBuf<int> dflag;
    buf.alloc((size_t)ld * 9 + (size_t)std::max(nProbe, 1) + 4);
    buf.zero(s);
    part.alloc((size_t)k::DYN_GRID_CAP * k::DYN_NV); amp.alloc(1); dflag.alloc(1);
    dflag.zero(s);
    double *dy = buf.p, *du = dy + ld, *duo = du + ld, *dvv = duo + ld, *dinv = dvv + ld, *dm = dinv + ld, *df = dm + ld, *da = df + ld, *dsnap = da + ld,
           *dprobe = dsnap + ld, *den = dprobe + std::max(nProbe, 1);
    upload(dy, y, n, s); upload(du, u, n, s); upload(dvv, v, n, s); upload(dinv, inv, n, s); upload(da, a, n, s);
    if (mass) upload(dm, mass, n, s);
    if (f) upload(df, f, n, s);
    upload(amp.p, &g, 1, s);
    if (nProbe) { dv.alloc((size_t)nProbe); MFH_HIP(hipMemcpyAsync(dv.p, probeVars, (size_t)nProbe * sizeof(int64_t), hipMemcpyHostToDevice, s)); }
    k::StepArgs sa{};
    sa.n = n; sa.dt = dt; sa.hdt = 0.5 * dt; sa.alpha = alpha; sa.den = 1.0 + alpha * (0.5 * dt);
    sa.mode = mode; sa.last = last ? 1 : 0; sa.step = 0; sa.wantEnergy = energies ? 1 : 0;
    sa.nProbe = nProbe; sa.amplitude = amp.p; sa.probeVars = dv.p; sa.probeRow = nProbe ? dprobe : nullptr; sa.snapRow = snapshot ? dsnap : nullptr; sa.flag = dflag.p;
    const int np = k::launch_explicit_step(sa, dy, du, duo, dvv, dinv, f ? df : nullptr, da, dm, part.p, std::max(1, std::min(c->dynGridCap, k::DYN_GRID_CAP)), s);
    if (energies) {
        const int col[4] = {0, 1, 2, 3};
        const double sc[4] = {0.5, 0.5, 1.0, 0.5};
        double *const dst[4] = {den, den + 1, den + 2, den + 3};
        k::launch_reduce(np, 4, col, sc, dst, part.p, k::dyn_open(), s);
        MFH_HIP(hipMemcpyAsync(energies, den, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    MFH_HIP(hipMemcpyAsync(u, last ? du : duo, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(v, dvv, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipMemcpyAsync(a, da, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (snapshot) MFH_HIP(hipMemcpyAsync(snapshot, dsnap, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (nProbe) MFH_HIP(hipMemcpyAsync(probeOut, dprobe, (size_t)nProbe * sizeof(double), hipMemcpyDeviceToHost, s));
    int h = 0;
    MFH_HIP(hipMemcpyAsync(&h, dflag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    *flag = h;
    MFH_CATCH(c)
}

// measurement (scripts/probe_explicit.py): average device time of `reps` launches of k_explicit_step (mode 0, loaded, no probes / snapshot / energies)
// on hashed vectors of n doubles, and of `reps` device-to-device copies that move the same bytes -- the kernel reads five vectors and writes two,
// a copy of 3.5 n doubles reads and writes as many -- in the same process
mfh_status mfh_time_explicit_step(mfh_ctx *c, int64_t n, int32_t reps, double *step_ms, double *copy_ms) {
    MFH_TRY(c)
    require(c && n >= 2 && reps > 0 && step_ms && copy_ms, MFH_ERR_INVALID, "mfh_time_explicit_step: arguments");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t ld = (n + 31) / 32 * 32;
    DBuf<double> buf, part;
    DBuf<int> dflag;
    buf.alloc((size_t)ld * 8);
    part.alloc((size_t)k::DYN_GRID_CAP * k::DYN_NV); dflag.alloc(1);
    dflag.zero(s);
    std::vector<double> h((size_t)ld * 8);
    for (size_t i = 0; i < h.size(); ++i) h[i] = 1e-3 * k::power_default_start((int64_t)i);
    upload(buf.p, h.data(), (int64_t)h.size(), s);
    double *y = buf.p, *u0 = y + ld, *u1 = u0 + ld, *v = u1 + ld, *inv = v + ld, *f = inv + ld, *a = f + ld;
    k::StepArgs sa{};
    sa.n = n; sa.dt = 1e-3; sa.hdt = 5e-4; sa.alpha = 0.1; sa.den = 1.0 + 0.1 * 5e-4; sa.flag = dflag.p;
    const int cap = std::max(1, std::min(c->dynGridCap, k::DYN_GRID_CAP));
    for (int r = 0; r < 3; ++r) k::launch_explicit_step(sa, y, r & 1 ? u1 : u0, r & 1 ? u0 : u1, v, inv, f, a, nullptr, part.p, cap, s);
    {
        EventTimer t(s);
        for (int r = 0; r < reps; ++r) k::launch_explicit_step(sa, y, r & 1 ? u1 : u0, r & 1 ? u0 : u1, v, inv, f, a, nullptr, part.p, cap, s);
        *step_ms = t.stop() / reps;
    }
    const size_t half = (size_t)(7 * n / 2) * sizeof(double);          // 3.5 n doubles from the first half of the buffer to the second
    MFH_HIP(hipMemcpyAsync(buf.p + 4 * ld, buf.p, half, hipMemcpyDeviceToDevice, s));
    {
        EventTimer t(s);
        for (int r = 0; r < reps; ++r) MFH_HIP(hipMemcpyAsync(buf.p + 4 * ld, buf.p, half, hipMemcpyDeviceToDevice, s));
        *copy_ms = t.stop() / reps;
    }
    MFH_CATCH(c)
}

// the HRZ weights of the context's element type as k_mass_hrz takes them (npe values; host work only)
mfh_status mfh_debug_hrz_weights(mfh_ctx *c, double *w) {
    MFH_TRY(c)
    require(c && w && c->haveMesh && !c->external, MFH_ERR_INVALID, "mfh_debug_hrz_weights: a context with a mesh and an output array");
    hrz_weights(c->tables, c->mesh.npe, w);
    MFH_CATCH(c)
}

// the absolute row sums of the element matrices, [nElem][npe][dim] (k_elem_abs_rowsums)
mfh_status mfh_debug_elem_abs_rowsums(mfh_ctx *c, double *out) {
    MFH_TRY(c)
    require(c && out, MFH_ERR_INVALID, "mfh_debug_elem_abs_rowsums: null argument");
    prepare_pencil(c, "mfh_debug_elem_abs_rowsums");
    ensure_geometry(c);
    const HostMesh &m = c->mesh;
    DBuf<double> rs;
    rs.alloc((size_t)m.nElem * (size_t)m.npe * (size_t)m.dim);
    k::launch_elem_abs_rowsums(asm_args(c), rs.p, 4 * std::max(1, std::min(c->dynGridCap, k::DYN_GRID_CAP)), c->stream);
    rs.download(out, rs.n, c->stream);
    MFH_CATCH(c)
}

}   // extern "C"
