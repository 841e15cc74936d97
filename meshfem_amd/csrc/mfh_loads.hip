// Volume loads (mfh_body_force_load, mfh_stress_field_load, include/meshfem_hip.h; docs/design/04_14_volume_loads.md): load vectors of fields that
// live in the interior of the body.
//   k_stress_field_load   f_i = sum_e sigma_e . int_e grad phi_i   (Simulator::perElementStressFieldLoad, LinearElasticity.hh:564-577 over
//                         perElementConstantStressLoad :135-151); sigma_e given, or C_e : eps_e of a given per-element strain
//   k_field_stress        C_e : eps_e per element, the array a caller subtracts from stressField(u) (thermal stress)
//   k_body_force_load     f_i = sum_e rho_e int_e phi_i b   with b one vector, one vector per element, or a nodal field interpolated with the mesh's own
//                         shape functions (no counterpart in the reference)
//   k_density_check       flags a density entry that is negative or not finite
// Gather form: one lane per DoF walks that DoF's (element, local node) pairs of the DoF-pair list (ensure_dof_pairs: code = e npe + i, grouped by
// dofForNode[node], ascending by element) and writes out[dof dim + c] once. No atomics of any kind: the order of the sum is the order of the list, so
// two calls return the same bits, and under a periodic DoF map the images of a DoF are added in a fixed order. A DoF without pairs gets 0.
#include "mfh_ctx.hh"
#include "mfh_device.hh"
#include "mfh_dispatch.hh"

namespace mfh { namespace k {

namespace {

constexpr int npe_of(int dim, int deg) { return dim == 3 ? (deg == 1 ? 4 : 10) : (deg == 1 ? 3 : 6); }

struct VolumeLoadArgs {
    int64_t nDoF;
    int geoStride, add;          // add: out += the sum (out = the sum otherwise)
    const int32_t *dofPtr, *dofPair;
    const double *geo;
    double intGrad[20];          // npe x {al, be}: int grad phi_i = vol (al gl[s_i] + be gl[t_i])
    double w[10];                // int phi_i / vol
    double b[3];                 // MFH_BODY_CONSTANT
};
struct MassTable { double m[100]; };   // int phi_i phi_j / vol, npe x npe (ShapeTables::massRef: the coefficients of the MAT_MASS assembly)

template <int DIM, int DEG, int MAT, bool STRAIN>
__global__ void __launch_bounds__(256) k_stress_field_load(VolumeLoadArgs a, const double *__restrict__ field, double *__restrict__ out) {
    constexpr int FL = DIM * (DIM + 1) / 2;
    constexpr int NPE = npe_of(DIM, DEG);
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < a.nDoF; r += (int64_t)gridDim.x * 256) {
        double acc[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
        const int last = a.dofPtr[r + 1];
        for (int q = a.dofPtr[r]; q < last; ++q) {
            const int64_t code = a.dofPair[q], e = code / NPE;
            const int i = (int)(code - e * NPE);
            const double *g = a.geo + e * a.geoStride;
            const double *f = field + e * FL;
            double sig[FL];
            if (STRAIN) {
                double sd[FL];
#pragma unroll
                for (int k = 0; k < FL; ++k) sd[k] = f[k] * (k < DIM ? 1.0 : 2.0);   // shearDoubled (ElasticityTensor.hh:437-441)
                elem_D_apply<DIM, MAT>(g, sd, sig);
            } else {
#pragma unroll
                for (int k = 0; k < FL; ++k) sig[k] = f[k];
            }
            const int si = sup_s<DIM, DEG>(i), ti = sup_t<DIM, DEG>(i);
            const double vol = g[12];
            // runtime-indexed kernel-argument array: read through a select chain over the small table
            double al = 0, be = 0;
#pragma unroll
            for (int k = 0; k < NPE; ++k) { al = (k == i) ? a.intGrad[2 * k] : al; be = (k == i) ? a.intGrad[2 * k + 1] : be; }
            double gi[DIM];
#pragma unroll
            for (int b = 0; b < DIM; ++b) gi[b] = vol * (al * g[si * DIM + b] + be * g[ti * DIM + b]);
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                double v = 0;
#pragma unroll
                for (int b = 0; b < DIM; ++b) v += sig[flat_idx<DIM>(c, b)] * gi[b];
                acc[c] += v;
            }
        }
#pragma unroll
        for (int c = 0; c < DIM; ++c) out[r * DIM + c] = a.add ? out[r * DIM + c] + acc[c] : acc[c];
    }
}

// one lane per element: every entry of out is written exactly once
template <int DIM, int MAT>
__global__ void __launch_bounds__(256) k_field_stress(int64_t nElem, const double *__restrict__ geo, int geoStride, const double *__restrict__ strain,
                                                     double *__restrict__ out) {
    constexpr int FL = DIM * (DIM + 1) / 2;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nElem; e += (int64_t)gridDim.x * 256) {
        double sd[FL], sig[FL];
#pragma unroll
        for (int k = 0; k < FL; ++k) sd[k] = strain[e * FL + k] * (k < DIM ? 1.0 : 2.0);
        elem_D_apply<DIM, MAT>(geo + e * geoStride, sd, sig);
#pragma unroll
        for (int k = 0; k < FL; ++k) out[e * FL + k] = sig[k];
    }
}

// KIND: MFH_BODY_CONSTANT (a.b), MFH_BODY_ELEMENT (b: [nElem][DIM]), MFH_BODY_NODE (b: [nNode][DIM], the element's nodes through elemNodes).
// The weights of a quadratic element are not all positive (w_vertex = 0 on triangles, -1/20 on tets): they are used as they are.
template <int DIM, int DEG, int KIND>
__global__ void __launch_bounds__(256) k_body_force_load(VolumeLoadArgs a, MassTable mt, const int32_t *__restrict__ elemNodes, const double *__restrict__ b,
                                                        const double *__restrict__ density, double *__restrict__ out) {
    constexpr int NPE = npe_of(DIM, DEG);
    __shared__ double mass[NPE * NPE];
    if (KIND == MFH_BODY_NODE) {
        // the lanes index the table by their local node: staged in LDS by one lane (constant indices into the kernel argument)
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < NPE * NPE; ++k) mass[k] = mt.m[k];
        }
        __syncthreads();
    }
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < a.nDoF; r += (int64_t)gridDim.x * 256) {
        double acc[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
        const int last = a.dofPtr[r + 1];
        for (int q = a.dofPtr[r]; q < last; ++q) {
            const int64_t code = a.dofPair[q], e = code / NPE;
            const int i = (int)(code - e * NPE);
            const double vol = a.geo[e * a.geoStride + 12];
            const double rv = density ? density[e] * vol : vol;
            if (KIND == MFH_BODY_NODE) {
                double s[DIM];
#pragma unroll
                for (int c = 0; c < DIM; ++c) s[c] = 0.0;
#pragma unroll
                for (int j = 0; j < NPE; ++j) {
                    const double m = mass[i * NPE + j];
                    const int64_t node = elemNodes[e * NPE + j];
#pragma unroll
                    for (int c = 0; c < DIM; ++c) s[c] += m * b[node * DIM + c];
                }
#pragma unroll
                for (int c = 0; c < DIM; ++c) acc[c] += rv * s[c];
            } else {
                double wi = 0;
#pragma unroll
                for (int k = 0; k < NPE; ++k) wi = (k == i) ? a.w[k] : wi;
                const double rw = rv * wi;
                if (KIND == MFH_BODY_CONSTANT) acc[0] += rw;     // the vector is a factor of the whole sum
                else {
#pragma unroll
                    for (int c = 0; c < DIM; ++c) acc[c] += rw * b[e * DIM + c];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            const double v = KIND == MFH_BODY_CONSTANT ? acc[0] * a.b[c] : acc[c];
            out[r * DIM + c] = a.add ? out[r * DIM + c] + v : v;
        }
    }
}

// flag[0] = 1 if some entry is negative, infinite or NaN (every lane that finds one stores the same value: no atomic needed)
__global__ void __launch_bounds__(256) k_density_check(int64_t n, const double *__restrict__ density, int *__restrict__ flag) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const double v = density[e];
        if (!(v >= 0.0) || v > 1.7976931348623157e308) flag[0] = 1;
    }
}

VolumeLoadArgs make_args(const AsmArgs &a, int64_t nDoF, const int32_t *dofPtr, const int32_t *dofPair, const ShapeTables &T, int add) {
    VolumeLoadArgs v{};
    v.nDoF = nDoF; v.geoStride = a.geoStride; v.add = add; v.dofPtr = dofPtr; v.dofPair = dofPair; v.geo = a.geo;
    for (int i = 0; i < a.npe; ++i) {
        v.intGrad[2 * i] = T.intGrad[(size_t)2 * i]; v.intGrad[2 * i + 1] = T.intGrad[(size_t)2 * i + 1];
        double w = 0;                                        // int phi_i = sum_j int phi_i phi_j (the shape functions sum to 1)
        for (int j = 0; j < a.npe; ++j) w += T.massRef[(size_t)i * a.npe + j];
        v.w[i] = w;
    }
    return v;
}

} // namespace

void launch_stress_field_load(const AsmArgs &a, int64_t nDoF, const int32_t *dofPtr, const int32_t *dofPair, const ShapeTables &T, int strainKind,
                              const double *field, int add, double *out, hipStream_t s) {
    if (nDoF <= 0) return;
    const VolumeLoadArgs v = make_args(a, nDoF, dofPtr, dofPair, T, add);
    const int grid = grid_for(nDoF);
    if (strainKind)
        with_elem(a, [&](auto D, auto G, auto M) { launch_k(k_stress_field_load<D(), G(), M(), true>, dim3(grid), dim3(256), 0, s, v, field, out); });
    else
        with_dim_deg(a.dim, a.deg, [&](auto D, auto G) { launch_k(k_stress_field_load<D(), G(), MAT_ISO, false>, dim3(grid), dim3(256), 0, s, v, field, out); });
    CHECK_LAUNCH();
}

void launch_field_stress(const AsmArgs &a, const double *strain, double *out, hipStream_t s) {
    if (a.nElem <= 0) return;
    const int grid = grid_for(a.nElem, 8192);
    with_dim(a.dim, [&](auto D) { with_elasticity(a.mat, [&](auto M) {
        launch_k(k_field_stress<D(), M()>, dim3(grid), dim3(256), 0, s, a.nElem, a.geo, a.geoStride, strain, out);
    }); });
    CHECK_LAUNCH();
}

void launch_body_force_load(const AsmArgs &a, int64_t nDoF, const int32_t *dofPtr, const int32_t *dofPair, const ShapeTables &T, int kind,
                            const int32_t *elemNodes, const double *b, const double *bConst, const double *density, int add, double *out, hipStream_t s) {
    if (nDoF <= 0) return;
    VolumeLoadArgs v = make_args(a, nDoF, dofPtr, dofPair, T, add);
    MassTable mt{};
    for (int k = 0; k < a.npe * a.npe; ++k) mt.m[k] = T.massRef[(size_t)k];
    if (kind == MFH_BODY_CONSTANT)
        for (int c = 0; c < a.dim; ++c) v.b[c] = bConst[c];
    const int grid = grid_for(nDoF);
    with_dim_deg(a.dim, a.deg, [&](auto D, auto G) { with_int<MFH_BODY_CONSTANT, MFH_BODY_ELEMENT, MFH_BODY_NODE>(kind, [&](auto K) {
        launch_k(k_body_force_load<D(), G(), K()>, dim3(grid), dim3(256), 0, s, v, mt, elemNodes, b, density, out);
    }); });
    CHECK_LAUNCH();
}

void launch_density_check(int64_t n, const double *density, int *flag, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_density_check, dim3(grid_for(n)), dim3(256), 0, s, n, density, flag);
    CHECK_LAUNCH();
}

}} // namespace mfh::k
