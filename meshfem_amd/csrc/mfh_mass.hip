// The density field of a context and the mass properties of the body (mfh_set_density, mfh_mass_properties, include/meshfem_hip.h;
// docs/design/04_15_density.md).
//   k_density_positive   flags a density entry that is not finite or not strictly positive (the lanes store the flag: no atomic)
//   k_mass_moments<1>    per-workgroup partials of {mass, first moments about the mesh's first vertex}
//   k_mass_moments<2>    per-workgroup partials of the second moments about the centre of mass of pass 1 (read from device memory: no host trip
//                        between the passes)
//   k_mass_finish<P>     one workgroup adds the partials of a pass in index order; pass 1 also forms the centre of mass
// Per straight-sided element with vertices p_k:  int 1 = vol,  int x = vol mean(p_k),
//   int (x - c)(x - c)^T = vol / ((d+1)(d+2)) (sum_k q_k q_k^T + (sum_k q_k)(sum_k q_k)^T),  q_k = p_k - c.
// The second moments are taken about the centre, not the origin: for a body far from the origin the latter cancel. No floating-point atomics:
// a lane adds its elements in index order, the lanes of a wave and the waves of a workgroup are added in a fixed tree, the workgroups in index
// order, and the grid depends on nElem only -- the same call returns the same bits.
#include "mfh_ctx.hh"
#include "mfh_device.hh"
#include "mfh_dispatch.hh"

namespace mfh { namespace k {

namespace {

__global__ void __launch_bounds__(256) k_density_positive(int64_t n, const double *__restrict__ density, int *__restrict__ flag) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const double v = density[e];
        if (!(v > 0.0) || v > 1.7976931348623157e308) flag[0] = 1;
    }
}

template <int DIM> DEV double simplex_volume(const double (&P)[DIM + 1][DIM]) {
    double E[DIM][DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k)
#pragma unroll
        for (int a = 0; a < DIM; ++a) E[k][a] = P[k + 1][a] - P[0][a];
    if (DIM == 2) return 0.5 * (E[0][0] * E[1][1] - E[0][1] * E[1][0]);
    return (E[0][0] * (E[1][1] * E[2][2] - E[1][2] * E[2][1]) - E[0][1] * (E[1][0] * E[2][2] - E[1][2] * E[2][0]) +
            E[0][2] * (E[1][0] * E[2][1] - E[1][1] * E[2][0])) * (1.0 / 6.0);
}

// props: {mass, com[DIM]} of pass 1 (PASS == 2 reads the centre from it). density may be null (= 1).
template <int DIM, int PASS>
__global__ void __launch_bounds__(256) k_mass_moments(int64_t nElem, const int32_t *__restrict__ elemNodes, int npe, const double *__restrict__ vertPos,
                                                     const double *__restrict__ density, const double *__restrict__ props,
                                                     double *__restrict__ partials) {
    constexpr int NV = PASS == 1 ? 1 + DIM : DIM * (DIM + 1) / 2;
    __shared__ double red[4 * NV];
    double c[DIM];
    if (PASS == 1) {
        const int64_t v0 = elemNodes[0];
#pragma unroll
        for (int a = 0; a < DIM; ++a) c[a] = vertPos[v0 * DIM + a];
    } else {
#pragma unroll
        for (int a = 0; a < DIM; ++a) c[a] = props[1 + a];
    }
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nElem; e += (int64_t)gridDim.x * 256) {
        double P[DIM + 1][DIM];
#pragma unroll
        for (int k = 0; k <= DIM; ++k) {
            const int64_t v = elemNodes[e * npe + k];
#pragma unroll
            for (int a = 0; a < DIM; ++a) P[k][a] = vertPos[v * DIM + a];
        }
        const double rv = (density ? density[e] : 1.0) * simplex_volume<DIM>(P);
        double sq[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            sq[a] = 0.0;
#pragma unroll
            for (int k = 0; k <= DIM; ++k) { P[k][a] -= c[a]; sq[a] += P[k][a]; }
        }
        if (PASS == 1) {
            acc[0] += rv;
#pragma unroll
            for (int a = 0; a < DIM; ++a) acc[1 + a] += rv * (sq[a] * (1.0 / (DIM + 1)));
        } else {
            const double w = rv * (1.0 / ((DIM + 1) * (DIM + 2)));
            int q = 0;
#pragma unroll
            for (int a = 0; a < DIM; ++a)
#pragma unroll
                for (int b = a; b < DIM; ++b, ++q) {
                    double t = sq[a] * sq[b];
#pragma unroll
                    for (int k = 0; k <= DIM; ++k) t += P[k][a] * P[k][b];
                    acc[q] += w * t;
                }
        }
    }
    block_sum<NV>(acc, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) partials[(int64_t)blockIdx.x * NV + k] = acc[k];
}

// out[k] = partials[0][k] + partials[1][k] + ... in that order. PASS 1: out = {scale mass, com}; PASS 2: out = scale {second moments}.
template <int DIM, int PASS>
__global__ void __launch_bounds__(64) k_mass_finish(int nPart, double scale, const double *__restrict__ partials, const int32_t *__restrict__ elemNodes,
                                                   const double *__restrict__ vertPos, double *__restrict__ out) {
    constexpr int NV = PASS == 1 ? 1 + DIM : DIM * (DIM + 1) / 2;
    __shared__ double tot[NV];
    if (threadIdx.x < NV) {
        double v = 0.0;
        for (int b = 0; b < nPart; ++b) v += partials[(int64_t)b * NV + threadIdx.x];
        tot[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x >= NV) return;
    if (PASS == 2) out[threadIdx.x] = scale * tot[threadIdx.x];
    else if (threadIdx.x == 0) out[0] = scale * tot[0];
    else out[threadIdx.x] = vertPos[(int64_t)elemNodes[0] * DIM + (threadIdx.x - 1)] + tot[threadIdx.x] / tot[0];
}

} // namespace

void launch_density_positive(int64_t n, const double *density, int *flag, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_density_positive, dim3(grid_for(n)), dim3(256), 0, s, n, density, flag);
    CHECK_LAUNCH();
}

int mass_moments_grid(int64_t nElem) { return grid_for(nElem, MASS_GRID_CAP); }

// props (device): {scale mass, com[dim]}; second (device): the upper triangle of scale S row by row; partials: scratch of MASS_PARTIALS doubles
void launch_mass_properties(int dim, int64_t nElem, const int32_t *elemNodes, int npe, const double *vertPos, const double *density, double scale,
                            double *partials, double *props, double *second, hipStream_t s) {
    const int grid = mass_moments_grid(nElem);
    with_dim(dim, [&](auto D) {
        launch_k(k_mass_moments<D(), 1>, dim3(grid), dim3(256), 0, s, nElem, elemNodes, npe, vertPos, density, (const double *)props, partials);
        launch_k(k_mass_finish<D(), 1>, dim3(1), dim3(64), 0, s, grid, scale, (const double *)partials, elemNodes, vertPos, props);
        launch_k(k_mass_moments<D(), 2>, dim3(grid), dim3(256), 0, s, nElem, elemNodes, npe, vertPos, density, (const double *)props, partials);
        launch_k(k_mass_finish<D(), 2>, dim3(1), dim3(64), 0, s, grid, scale, (const double *)partials, elemNodes, vertPos, second);
    });
    CHECK_LAUNCH();
}

}} // namespace mfh::k

using namespace mfh;
using namespace mfhi;

namespace {
// the contexts a density field and the mass properties are defined on: a mesh on a device, all rows owned (modes and dynamics refuse the rest too)
void require_density_context(mfh_ctx *c) {
    require(c && c->haveMesh && !c->hostOnly && !c->external, MFH_ERR_STATE, "the density field needs a mesh on a device");
    require(!dist_active(c) && c->mesh.nOwned == c->mesh.nNode, MFH_ERR_UNSUPPORTED, "the density field: unpartitioned contexts only");
    require(c->mesh.dim == 2 || c->mesh.dim == 3, MFH_ERR_UNSUPPORTED, "2D / 3D meshes");
}
} // namespace

extern "C" {

mfh_status mfh_set_density(mfh_ctx *c, const double *rho, int64_t n, int32_t flags) {
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_set_density: null context");
    require_density_context(c);
    require((flags & ~MFH_LOAD_ON_DEVICE) == 0, MFH_ERR_INVALID, "flags: 0 | MFH_LOAD_ON_DEVICE");
    if (!rho) {                                  // back to unit density
        if (c->haveDensity) clear_density(c);
        return MFH_OK;
    }
    const int64_t nElem = c->mesh.nElem;
    require(n == nElem, MFH_ERR_INVALID, "mfh_set_density: one value per element");
    const bool onDevice = (flags & MFH_LOAD_ON_DEVICE) != 0;
    MFH_HIP(hipSetDevice(c->device));
    bool bad = false;
    if (!onDevice) {
        for (int64_t e = 0; e < n && !bad; ++e) bad = !(rho[e] > 0.0) || !std::isfinite(rho[e]);
    } else {
        DBuf<int> flag;
        flag.alloc(1);
        flag.zero(c->stream);
        k::launch_density_positive(n, rho, flag.p, c->stream);
        int h = 0;
        flag.download(&h, 1, c->stream);
        bad = h != 0;
    }
    require(!bad, MFH_ERR_INVALID, "mfh_set_density: an entry is not finite or not strictly positive (the mass matrix must stay positive definite)");
    // a buffer of its own every time: the field in force stays untouched until the new one is complete
    DBuf<double> fresh;
    fresh.alloc((size_t)n);
    MFH_HIP(hipMemcpyAsync(fresh.p, rho, (size_t)n * sizeof(double), onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    MFH_HIP(hipStreamSynchronize(c->stream));
    c->dDensity.swap(fresh);
    c->haveDensity = true;
    ++c->densityGen;
    MFH_CATCH(c)
}

mfh_status mfh_mass_properties(mfh_ctx *c, double scale, double *mass, double *com, double *S, int32_t flags) {
    MFH_TRY(c)
    require(c != nullptr, MFH_ERR_INVALID, "mfh_mass_properties: null context");
    require_density_context(c);
    require(scale > 0.0 && std::isfinite(scale), MFH_ERR_INVALID, "mfh_mass_properties: scale > 0");
    require(flags == 0, MFH_ERR_INVALID, "mfh_mass_properties: flags is reserved and must be 0 (the outputs are host pointers)");
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);                          // (refuses inverted elements: the volumes below are signed)
    const HostMesh &m = c->mesh;
    const int d = m.dim;
    DBuf<double> part, res;
    part.alloc((size_t)k::MASS_PARTIALS);
    res.alloc(16);                               // {mass, com} from entry 0, the upper triangle of S from entry 8
    res.zero(c->stream);
    k::launch_mass_properties(d, m.nElem, c->dElemNodes.p, m.npe, c->dVertPos.p, c->haveDensity ? c->dDensity.p : nullptr, scale, part.p, res.p, res.p + 8,
                              c->stream);
    double h[16];
    res.download(h, 16, c->stream);
    if (mass) *mass = h[0];
    if (com)
        for (int a = 0; a < d; ++a) com[a] = h[1 + a];
    if (S) {
        int q = 0;
        for (int a = 0; a < d; ++a)
            for (int b = a; b < d; ++b, ++q) S[a * d + b] = S[b * d + a] = h[8 + q];
    }
    MFH_CATCH(c)
}

// measurement (meshfem_hip_extras.h): the mass assembly pass into the resident buffer, unit density and -- with a field set -- density-weighted,
// launched in turns so that both see the same state of the machine
mfh_status mfh_time_mass_assembly(mfh_ctx *c, int32_t reps, double *unit_ms, double *field_ms) {
    MFH_TRY(c)
    require(c && unit_ms && reps > 0, MFH_ERR_INVALID, "bad arguments");
    require_density_context(c);
    require(!field_ms || c->haveDensity, MFH_ERR_STATE, "mfh_time_mass_assembly: no density field set");
    MFH_HIP(hipSetDevice(c->device));
    ensure_mass(c);                              // geometry, pattern (both triangles: option matrix_storage 0), the buffer
    k::AsmArgs a = asm_args(c);
    a.vals = c->dMassVals.p;
    for (int r = 0; r < reps; ++r) {
        a.mat = MAT_MASS; a.density = nullptr;
        { EventTimer t(c->stream); k::launch_assemble_gather(a, c->stream); unit_ms[r] = t.stop(); }
        if (!field_ms) continue;
        a.mat = MAT_MASS_RHO; a.density = c->dDensity.p;
        { EventTimer t(c->stream); k::launch_assemble_gather(a, c->stream); field_ms[r] = t.stop(); }
    }
    c->massDensityGen = -1;                      // (the buffer holds the last pass: the next consumer reassembles)
    MFH_CATCH(c)
}

}   // extern "C"
