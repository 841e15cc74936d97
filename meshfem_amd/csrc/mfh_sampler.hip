// Field sampler on the device (FieldSampler.hh of the reference: closestElementAndPoint / closestElementAndBaryCoords / closestNodeAndSqDist /
// contains / sample), docs/design/04_11_field_sampler.md. Where the reference walks a libigl AABB tree on the host, this file builds a uniform
// cell grid with one radix sort and walks it with one lane per query point:
//   index      k_grid_count / k_grid_fill (one 64-bit key cell << 32 | item per cell an item's inflated bounding box overlaps), rocPRIM radix sort,
//              k_cell_start (binary search of every cell's first key), k_grid_items. Every cell's list is ascending in item index.
//   k_locate   the first element of the point's cell with min lambda >= -1e-12 (so: the LOWEST index of all elements that contain the point)
//   k_closest_boundary   the flagged (not contained) points: closest boundary element in expanding shells of cells, total order
//              (squared distance, boundary element index); element = the boundary element's parent
//   k_sample_field / k_closest_node   evaluation at (element, barycentric coordinates)
// FP64 throughout, no floating-point atomics (the one atomic is an integer OR that says "some point was not contained"): the same call on the
// same context returns the same bits.
#include "mfh_ctx.hh"
#include "mfh_device.hh"
#include "mfh_dispatch.hh"
#include <rocprim/rocprim.hpp>

namespace mfh { namespace k {

namespace {

constexpr int SAMPLER_BUILD_GRID_CAP = 1024;   // workgroups of the build kernels (grid-stride above 262 144 items)
constexpr int SAMPLER_POINT_GRID_CAP = 4096;   // workgroups of the per-point kernels (grid-stride above 1 048 576 points)
constexpr double CONTAIN_TOL = 1e-12;          // contains(p, lambda, 1e-12) of the reference

struct GridDesc {
    int nc[3];
    double org[3], hi[3], cs[3], inv[3];
    const int32_t *cellStart, *items;
};
struct EdgeTable { int s[6], t[6]; };          // kEdgeStart / kEdgeEnd (the local vertices of edge node j)

// cell of coordinate x along axis a, clamped into the grid. Monotone in x: the cells of an item's box [lo, hi] bracket the cell of every point in it.
DEV int cell_of(const GridDesc &g, int a, double x) {
    double t = (x - g.org[a]) * g.inv[a];
    t = fmin(fmax(t, 0.0), (double)(g.nc[a] - 1));
    return (int)t;
}

template <int DIM>
DEV void item_cells(const GridDesc &g, const int32_t *iv, int nv, const double *__restrict__ pos, double pad, int lo[3], int hi[3]) {
    double mn[DIM], mx[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) { mn[a] = pos[(size_t)iv[0] * DIM + a]; mx[a] = mn[a]; }
    for (int k2 = 1; k2 < nv; ++k2)
#pragma unroll
        for (int a = 0; a < DIM; ++a) { const double x = pos[(size_t)iv[k2] * DIM + a]; mn[a] = fmin(mn[a], x); mx[a] = fmax(mx[a], x); }
    lo[2] = hi[2] = 0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) { lo[a] = cell_of(g, a, mn[a] - pad); hi[a] = cell_of(g, a, mx[a] + pad); }
}

// items: rows of `verts` (stride ints apart, the first nv are vertex ids into pos). cnt[i] = cells item i is entered in.
template <int DIM>
__global__ void __launch_bounds__(256) k_grid_count(int64_t n, const int32_t *__restrict__ verts, int stride, int nv, const double *__restrict__ pos, GridDesc g,
                                                    double pad, unsigned long long *__restrict__ cnt) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int lo[3], hi[3];
        item_cells<DIM>(g, verts + i * stride, nv, pos, pad, lo, hi);
        cnt[i] = (unsigned long long)(hi[0] - lo[0] + 1) * (unsigned long long)(hi[1] - lo[1] + 1) * (unsigned long long)(hi[2] - lo[2] + 1);
    }
}
// the same walk writes the keys: item i owns key[off[i] .. off[i + 1])
template <int DIM>
__global__ void __launch_bounds__(256) k_grid_fill(int64_t n, const int32_t *__restrict__ verts, int stride, int nv, const double *__restrict__ pos, GridDesc g,
                                                   double pad, const unsigned long long *__restrict__ off, unsigned long long *__restrict__ key) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int lo[3], hi[3];
        item_cells<DIM>(g, verts + i * stride, nv, pos, pad, lo, hi);
        unsigned long long w = off[i];
        const unsigned long long end = off[i + 1];
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int x = lo[0]; x <= hi[0]; ++x) {
                    const unsigned long long cell = ((unsigned long long)z * g.nc[1] + y) * g.nc[0] + x;
                    if (w < end) key[w] = (cell << 32) | (unsigned long long)i;
                    ++w;
                }
    }
}
// cellStart[c] = index of the first sorted key of a cell >= c (c = nCells gives nPairs)
__global__ void __launch_bounds__(256) k_cell_start(int64_t nCells, int64_t nPairs, const unsigned long long *__restrict__ key, int32_t *__restrict__ cellStart) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c <= nCells; c += (int64_t)gridDim.x * 256) {
        const unsigned long long want = (unsigned long long)c << 32;
        int64_t lo = 0, hi = nPairs;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (key[mid] < want) lo = mid + 1; else hi = mid;
        }
        cellStart[c] = (int32_t)lo;
    }
}
__global__ void __launch_bounds__(256) k_grid_items(int64_t nPairs, const unsigned long long *__restrict__ key, int32_t *__restrict__ items) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nPairs; i += (int64_t)gridDim.x * 256) items[i] = (int32_t)(key[i] & 0xffffffffull);
}

// lambda_k = delta_k0 + gl_k . (p - x_v0) from the element record (gl[k dim + a]) and the position of the element's vertex 0
template <int DIM>
DEV double bary_in_element(const double *__restrict__ rec, const double *__restrict__ x0, const double *p, double *lam) {
    double d[DIM], mn = 0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) d[a] = p[a] - x0[a];
#pragma unroll
    for (int k2 = 0; k2 <= DIM; ++k2) {
        double l = k2 == 0 ? 1.0 : 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) l += rec[k2 * DIM + a] * d[a];
        lam[k2] = l;
        mn = k2 == 0 ? l : fmin(mn, l);
    }
    return mn;
}

// flag: 0 contained, 1 not contained (k_closest_boundary finishes the point), 2 a coordinate is not finite (element -1, NaN everywhere)
template <int DIM>
__global__ void __launch_bounds__(256) k_locate(int64_t nP, const double *__restrict__ P, GridDesc g, const int32_t *__restrict__ elemNodes, int npe,
                                                const double *__restrict__ pos, const double *__restrict__ geo, int geoStride, int32_t *__restrict__ elem,
                                                double *__restrict__ bary, double *__restrict__ closest, double *__restrict__ sqDist,
                                                uint8_t *__restrict__ flag, int *__restrict__ anyOutside) {
    const double nan = __builtin_nan("");
    bool any = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nP; i += (int64_t)gridDim.x * 256) {
        double p[DIM], lam[DIM + 1];
        bool finite = true, inBox = true;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            p[a] = P[i * DIM + a];
            finite = finite && isfinite(p[a]);
            inBox = inBox && p[a] >= g.org[a] && p[a] <= g.hi[a];
        }
        int32_t found = -1;
        if (finite && inBox) {
            int64_t cell = 0;
#pragma unroll
            for (int a = DIM - 1; a >= 0; --a) cell = cell * g.nc[a] + cell_of(g, a, p[a]);
            const int32_t jEnd = g.cellStart[cell + 1];
            for (int32_t j = g.cellStart[cell]; j < jEnd; ++j) {
                const int32_t e = g.items[j];
                const int32_t v0 = elemNodes[(int64_t)e * npe];
                if (bary_in_element<DIM>(geo + (int64_t)e * geoStride, pos + (int64_t)v0 * DIM, p, lam) >= -CONTAIN_TOL) { found = e; break; }
            }
        }
        elem[i] = found;
        flag[i] = finite ? (found >= 0 ? 0 : 1) : 2;
        any = any || (finite && found < 0);
        // (a point that is not contained keeps NaN unless k_closest_boundary finds a boundary element for it)
#pragma unroll
        for (int k2 = 0; k2 <= DIM; ++k2) if (bary) bary[i * (DIM + 1) + k2] = found >= 0 ? lam[k2] : nan;
#pragma unroll
        for (int a = 0; a < DIM; ++a) if (closest) closest[i * DIM + a] = found >= 0 ? p[a] : nan;
        if (sqDist) sqDist[i] = found >= 0 ? 0.0 : nan;
    }
    if (__syncthreads_or(any ? 1 : 0) && threadIdx.x == 0) atomicOr(anyOutside, 1);     // one integer atomic per workgroup
}

// closest point of the segment (a, b) to p
DEV void closest_on_simplex(const double *p, const double (*v)[2], double *c) {
    const double ab[2] = {v[1][0] - v[0][0], v[1][1] - v[0][1]};
    const double len2 = ab[0] * ab[0] + ab[1] * ab[1];
    double t = len2 > 0 ? ((p[0] - v[0][0]) * ab[0] + (p[1] - v[0][1]) * ab[1]) / len2 : 0.0;
    t = fmin(fmax(t, 0.0), 1.0);
    c[0] = v[0][0] + t * ab[0];
    c[1] = v[0][1] + t * ab[1];
}
DEV double dot3(const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }
// closest point of the triangle (a, b, c) to p: classification into the vertex, edge and face regions
DEV void closest_on_simplex(const double *p, const double (*v)[3], double *out) {
    const double *a = v[0], *b = v[1], *c = v[2];
    double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { ab[q] = b[q] - a[q]; ac[q] = c[q] - a[q]; ap[q] = p[q] - a[q]; bp[q] = p[q] - b[q]; cp[q] = p[q] - c[q]; }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    if (d1 <= 0 && d2 <= 0) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; return; }
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    if (d3 >= 0 && d4 <= d3) { out[0] = b[0]; out[1] = b[1]; out[2] = b[2]; return; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0 && d1 >= 0 && d3 <= 0) {
        const double t = d1 / (d1 - d3);
#pragma unroll
        for (int q = 0; q < 3; ++q) out[q] = a[q] + t * ab[q];
        return;
    }
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d6 >= 0 && d5 <= d6) { out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; return; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0 && d2 >= 0 && d6 <= 0) {
        const double t = d2 / (d2 - d6);
#pragma unroll
        for (int q = 0; q < 3; ++q) out[q] = a[q] + t * ac[q];
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) {
        const double t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
        for (int q = 0; q < 3; ++q) out[q] = b[q] + t * (c[q] - b[q]);
        return;
    }
    const double den = 1.0 / (va + vb + vc), s = vb * den, t = vc * den;
#pragma unroll
    for (int q = 0; q < 3; ++q) out[q] = a[q] + ab[q] * s + ac[q] * t;
}

template <int DIM> struct Best { double d2; int32_t idx; double c[DIM]; };

template <int DIM>
DEV void visit_cell(const GridDesc &g, int64_t cell, const int32_t *__restrict__ bdryVerts, const double *__restrict__ pos, const double *p, Best<DIM> &best) {
    const int32_t jEnd = g.cellStart[cell + 1];
    for (int32_t j = g.cellStart[cell]; j < jEnd; ++j) {
        const int32_t b = g.items[j];
        double v[DIM][DIM], c[DIM];
#pragma unroll
        for (int k2 = 0; k2 < DIM; ++k2) {
            const int32_t n = bdryVerts[(int64_t)b * DIM + k2];
#pragma unroll
            for (int a = 0; a < DIM; ++a) v[k2][a] = pos[(int64_t)n * DIM + a];
        }
        closest_on_simplex(p, v, c);
        double d2 = 0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) d2 += (p[a] - c[a]) * (p[a] - c[a]);
        // total order (squared distance, boundary element index)
        if (best.idx < 0 || d2 < best.d2 || (d2 == best.d2 && b < best.idx)) {
            best.d2 = d2; best.idx = b;
#pragma unroll
            for (int a = 0; a < DIM; ++a) best.c[a] = c[a];
        }
    }
}

// The flagged points only (launched over all points, the others return at once). Shells r = 0, 1, ... of cells around the cell nearest to p; after
// shell r every boundary element that meets the block of cells within r of the centre has been seen, and whatever has not lies beyond one of the
// block's sides that are still inside the grid: at least sqrt(gap^2 + (distance of p to the mesh's inflated bounding box along the other axes)^2) away. The search
// ends when the best squared distance is below the smallest such bound, or when no side is left inside the grid -- after at most
// max(nc) shells, whatever p is.
template <int DIM>
__global__ void __launch_bounds__(256) k_closest_boundary(int64_t nP, const double *__restrict__ P, const uint8_t *__restrict__ flag, GridDesc g,
                                                          const int32_t *__restrict__ bdryVerts, const int32_t *__restrict__ bdryParent,
                                                          const int32_t *__restrict__ elemNodes, int npe, const double *__restrict__ pos,
                                                          const double *__restrict__ geo, int geoStride, int32_t *__restrict__ elem, double *__restrict__ bary,
                                                          double *__restrict__ closest, double *__restrict__ sqDist) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nP; i += (int64_t)gridDim.x * 256) {
        if (flag[i] != 1) continue;
        double p[DIM], dbox[DIM];
        int cc[3] = {0, 0, 0}, rMax = 0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            p[a] = P[i * DIM + a];
            cc[a] = cell_of(g, a, p[a]);
            rMax = max(rMax, max(cc[a], g.nc[a] - 1 - cc[a]));
            dbox[a] = fmax(fmax(g.org[a] - p[a], p[a] - g.hi[a]), 0.0);      // to the inflated bounding box, which holds every item (the last cells overhang it)
        }
        Best<DIM> best;
        best.d2 = 0; best.idx = -1;
        for (int r = 0; r <= rMax; ++r) {
            const int z0 = DIM == 3 ? max(cc[2] - r, 0) : 0, z1 = DIM == 3 ? min(cc[2] + r, g.nc[2] - 1) : 0;
            const int y0 = max(cc[1] - r, 0), y1 = min(cc[1] + r, g.nc[1] - 1);
            const int x0 = max(cc[0] - r, 0), x1 = min(cc[0] + r, g.nc[0] - 1);
            for (int z = z0; z <= z1; ++z) {
                const bool zFace = DIM == 3 && abs(z - cc[2]) == r;
                for (int y = y0; y <= y1; ++y) {
                    const int64_t row = ((int64_t)z * g.nc[1] + y) * g.nc[0];
                    if (zFace || abs(y - cc[1]) == r) {
                        for (int x = x0; x <= x1; ++x) visit_cell<DIM>(g, row + x, bdryVerts, pos, p, best);
                    } else {      // (r > 0 here) the two cells of this row on the shell
                        if (cc[0] - r >= 0) visit_cell<DIM>(g, row + cc[0] - r, bdryVerts, pos, p, best);
                        if (cc[0] + r <= g.nc[0] - 1) visit_cell<DIM>(g, row + cc[0] + r, bdryVerts, pos, p, best);
                    }
                }
            }
            bool open = false;
            double bound = 0;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                double other = 0;
#pragma unroll
                for (int b = 0; b < DIM; ++b) if (b != a) other += dbox[b] * dbox[b];
                if (cc[a] - r > 0) {
                    const double gap = fmax(p[a] - (g.org[a] + (cc[a] - r) * g.cs[a]), 0.0), bd = gap * gap + other;
                    bound = open ? fmin(bound, bd) : bd; open = true;
                }
                if (cc[a] + r < g.nc[a] - 1) {
                    const double gap = fmax(g.org[a] + (cc[a] + r + 1) * g.cs[a] - p[a], 0.0), bd = gap * gap + other;
                    bound = open ? fmin(bound, bd) : bd; open = true;
                }
            }
            if (!open) break;
            if (best.idx >= 0 && best.d2 < bound) break;      // strictly: an unseen element at exactly the best distance could have the lower index
        }
        if (best.idx < 0) continue;     // a mesh without boundary elements: k_locate's element -1 and NaN stay
        const int32_t e = bdryParent[best.idx];
        const int32_t v0 = elemNodes[(int64_t)e * npe];
        double lam[DIM + 1];
        bary_in_element<DIM>(geo + (int64_t)e * geoStride, pos + (int64_t)v0 * DIM, best.c, lam);
        elem[i] = e;
#pragma unroll
        for (int k2 = 0; k2 <= DIM; ++k2) if (bary) bary[i * (DIM + 1) + k2] = lam[k2];
#pragma unroll
        for (int a = 0; a < DIM; ++a) if (closest) closest[i * DIM + a] = best.c[a];
        if (sqDist) sqDist[i] = best.d2;
    }
}

// the degree's shape functions at barycentric coordinates lam: P1 lambda_k; P2 lambda_k (2 lambda_k - 1) at the vertices, 4 lambda_s lambda_t at
// the node of edge (s, t)
template <int DIM, int DEG> DEV void shape_functions(const double *lam, const EdgeTable &et, double *w) {
    constexpr int NE = DIM == 2 ? 3 : 6;
    if (DEG == 1) {
#pragma unroll
        for (int k2 = 0; k2 <= DIM; ++k2) w[k2] = lam[k2];
    } else {
#pragma unroll
        for (int k2 = 0; k2 <= DIM; ++k2) w[k2] = lam[k2] * (2.0 * lam[k2] - 1.0);
#pragma unroll
        for (int j = 0; j < NE; ++j) w[DIM + 1 + j] = 4.0 * lam[et.s[j]] * lam[et.t[j]];
    }
}

// kind 0: per-vertex field, 1: per-element, 2: per-node (MeshFieldSampler::sample). field: rows of nComp interleaved components.
template <int DIM, int DEG>
__global__ void __launch_bounds__(256) k_sample_field(int64_t nP, const int32_t *__restrict__ elem, const double *__restrict__ bary,
                                                      const int32_t *__restrict__ elemNodes, EdgeTable et, int kind, const double *__restrict__ field, int nComp,
                                                      double *__restrict__ out) {
    constexpr int NPE = DEG == 1 ? DIM + 1 : (DIM == 2 ? 6 : 10);
    const double nan = __builtin_nan("");
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nP; i += (int64_t)gridDim.x * 256) {
        const int32_t e = elem[i];
        double *o = out + i * nComp;
        if (e < 0) { for (int c = 0; c < nComp; ++c) o[c] = nan; continue; }
        if (kind == 1) { for (int c = 0; c < nComp; ++c) o[c] = field[(int64_t)e * nComp + c]; continue; }
        double lam[DIM + 1], w[NPE];
        int32_t row[NPE];
#pragma unroll
        for (int k2 = 0; k2 <= DIM; ++k2) lam[k2] = bary[i * (DIM + 1) + k2];
        int n = DIM + 1;
        if (kind == 0 || DEG == 1) {
#pragma unroll
            for (int k2 = 0; k2 <= DIM; ++k2) w[k2] = lam[k2];
        } else {
            shape_functions<DIM, DEG>(lam, et, w);
            n = NPE;
        }
#pragma unroll
        for (int j = 0; j < NPE; ++j) if (j < n) row[j] = elemNodes[(int64_t)e * NPE + j];
        for (int c = 0; c < nComp; ++c) {
            double s = 0;
#pragma unroll
            for (int j = 0; j < NPE; ++j) if (j < n) s += w[j] * field[(int64_t)row[j] * nComp + c];
            o[c] = s;
        }
    }
}

// the node whose shape function is largest at the point's barycentric coordinates (lowest local index on ties) and its squared distance to p
template <int DIM, int DEG>
__global__ void __launch_bounds__(256) k_closest_node(int64_t nP, const double *__restrict__ P, const int32_t *__restrict__ elem, const double *__restrict__ bary,
                                                      const int32_t *__restrict__ elemNodes, EdgeTable et, const double *__restrict__ pos,
                                                      int32_t *__restrict__ node, double *__restrict__ sqDist) {
    constexpr int NPE = DEG == 1 ? DIM + 1 : (DIM == 2 ? 6 : 10);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nP; i += (int64_t)gridDim.x * 256) {
        const int32_t e = elem[i];
        if (e < 0) { if (node) node[i] = -1; if (sqDist) sqDist[i] = __builtin_nan(""); continue; }
        double lam[DIM + 1], w[NPE];
#pragma unroll
        for (int k2 = 0; k2 <= DIM; ++k2) lam[k2] = bary[i * (DIM + 1) + k2];
        shape_functions<DIM, DEG>(lam, et, w);
        int jb = 0;
#pragma unroll
        for (int j = 1; j < NPE; ++j) if (w[j] > w[jb]) jb = j;
        const int32_t n = elemNodes[(int64_t)e * NPE + jb];
        double d2 = 0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) { const double d = pos[(int64_t)n * DIM + a] - P[i * DIM + a]; d2 += d * d; }
        if (node) node[i] = n;
        if (sqDist) sqDist[i] = d2;
    }
}

inline unsigned bits_for(uint64_t v) { unsigned b = 1; while ((v >> b) != 0 && b < 32) ++b; return b; }

GridDesc grid_desc(const mfh_ctx::SamplerGrid &G) {
    GridDesc g{};
    for (int a = 0; a < 3; ++a) { g.nc[a] = G.nc[a]; g.org[a] = G.org[a]; g.hi[a] = G.hi[a]; g.cs[a] = G.cs[a]; g.inv[a] = 1.0 / G.cs[a]; }
    g.cellStart = G.cellStart.p;
    g.items = G.items.p;
    return g;
}
EdgeTable edge_table(int dim) {
    EdgeTable et{};
    for (int j = 0; j < (dim == 2 ? 3 : 6); ++j) { et.s[j] = kEdgeStart[j]; et.t[j] = kEdgeEnd[j]; }
    return et;
}

// the ladders of this file end the other way round: a dimension other than 2 is 3, a degree other than 1 is 2
template <class F> static void with_dim23(int dim, F &&f) { with_int<2, 3>(dim, f); }
template <class F> static void with_dim23_deg(int dim, int deg, F &&f) {
    with_dim23(dim, [&](auto D) { with_int<1, 2>(deg, [&](auto G) { f(D, G); }); });
}

// One grid over `n` items (rows of dVerts / hVerts, `stride` ints apart, the first nv entries vertex ids): cell sizes = scale x the mean
// bounding-box extent of the items per axis, doubled until the pair count is at most 32 n and below 2^31 and the grid has at most 8 n + 4096
// cells (bounded: one cell holds n pairs).
void build_grid(mfh_ctx *c, mfh_ctx::SamplerGrid &G, int64_t n, const int32_t *dVerts, const int32_t *hVerts, int stride, int nv, const double *bbMin,
                const double *bbMax, double pad) {
    const HostMesh &m = c->mesh;
    const int dim = m.dim;
    hipStream_t s = c->stream;
    const double t0 = now_ms();
    G.reset();
    G.nItems = n;
    double mean[3] = {0, 0, 0}, ext[3] = {1, 1, 1};
    for (int64_t i = 0; i < n; ++i) {
        const int32_t *iv = hVerts + i * stride;
        for (int a = 0; a < dim; ++a) {
            double mn = m.vertPos[(size_t)iv[0] * dim + a], mx = mn;
            for (int k2 = 1; k2 < nv; ++k2) { const double x = m.vertPos[(size_t)iv[k2] * dim + a]; mn = std::min(mn, x); mx = std::max(mx, x); }
            mean[a] += mx - mn;
        }
    }
    G.hostMs = now_ms() - t0;
    for (int a = 0; a < 3; ++a) {
        G.org[a] = a < dim ? bbMin[a] - pad : 0.0;
        G.hi[a] = a < dim ? bbMax[a] + pad : 0.0;
        ext[a] = a < dim ? G.hi[a] - G.org[a] : 1.0;
        double cs = a < dim && n > 0 ? c->samplerCellScale * mean[a] / (double)n : ext[a];
        if (!(cs > 0) || !std::isfinite(cs)) cs = ext[a];          // every item flat along this axis: one cell
        if (!(ext[a] > 0)) { ext[a] = 1.0; cs = 1.0; }               // a mesh without extent along this axis (or no items at all)
        G.cs[a] = std::max(cs, ext[a] / 2097152.0);
    }
    DBuf<unsigned long long> cnt, off;
    DBuf<char> tmp;
    int64_t total = 0;
    if (n > 0) { cnt.alloc((size_t)n + 1); off.alloc((size_t)n + 1); }
    for (;;) {
        double cells = 1;
        for (int a = 0; a < 3; ++a) {
            const double ncd = a < dim ? std::max(1.0, std::ceil(ext[a] / G.cs[a])) : 1.0;
            G.nc[a] = (int)std::min(ncd, 4194304.0);
            cells *= (double)G.nc[a];
        }
        const bool oneCell = G.nc[0] == 1 && G.nc[1] == 1 && G.nc[2] == 1;
        bool ok = cells <= 8.0 * (double)n + 4096.0;
        if (ok && n > 0) {
            const GridDesc g = grid_desc(G);
            MFH_HIP(hipMemsetAsync(cnt.p + n, 0, sizeof(unsigned long long), s));
            const int grid = grid_for(n, SAMPLER_BUILD_GRID_CAP);
            with_dim23(dim, [&](auto D) { launch_k(k_grid_count<D()>, dim3(grid), dim3(256), 0, s, n, dVerts, stride, nv, c->dVertPos.p, g, pad, cnt.p); });
            CHECK_LAUNCH();
            size_t bytes = 0;
            MFH_HIP(rocprim::exclusive_scan(nullptr, bytes, cnt.p, off.p, 0ull, (size_t)n + 1, rocprim::plus<unsigned long long>(), s));
            if (bytes + 16 > tmp.n) tmp.alloc(bytes + 16);
            MFH_HIP(rocprim::exclusive_scan(tmp.p, bytes, cnt.p, off.p, 0ull, (size_t)n + 1, rocprim::plus<unsigned long long>(), s));
            unsigned long long h = 0;
            MFH_HIP(hipMemcpyAsync(&h, off.p + n, sizeof(h), hipMemcpyDeviceToHost, s));
            MFH_HIP(hipStreamSynchronize(s));
            ok = h <= 32ull * (unsigned long long)n && h <= 2147483647ull;
            total = (int64_t)h;
        }
        if (ok || oneCell) break;
        for (int a = 0; a < dim; ++a) G.cs[a] *= 2.0;
    }
    mfhi::require(total <= 2147483647LL, MFH_ERR_UNSUPPORTED, "field sampler: more than 2^31 items in one cell grid");
    const int64_t nCells = (int64_t)G.nc[0] * G.nc[1] * G.nc[2];
    G.nPairs = total;
    G.cellStart.alloc((size_t)nCells + 1);
    if (total > 0) {
        const GridDesc g = grid_desc(G);
        DBuf<unsigned long long> keyA, keyB;
        keyA.alloc((size_t)total); keyB.alloc((size_t)total);
        const int grid = grid_for(n, SAMPLER_BUILD_GRID_CAP);
        with_dim23(dim, [&](auto D) {
            launch_k(k_grid_fill<D()>, dim3(grid), dim3(256), 0, s, n, dVerts, stride, nv, c->dVertPos.p, g, pad, off.p,
                     keyA.p);
        });
        CHECK_LAUNCH();
        const unsigned endBit = 32 + bits_for((uint64_t)nCells);
        size_t bytes = 0;
        MFH_HIP(rocprim::radix_sort_keys(nullptr, bytes, keyA.p, keyB.p, (size_t)total, 0u, endBit, s));
        if (bytes + 16 > tmp.n) tmp.alloc(bytes + 16);
        MFH_HIP(rocprim::radix_sort_keys(tmp.p, bytes, keyA.p, keyB.p, (size_t)total, 0u, endBit, s));
        G.items.alloc((size_t)total);
        hipLaunchKernelGGL(k_cell_start, dim3(grid_for(nCells + 1, SAMPLER_BUILD_GRID_CAP)), dim3(256), 0, s, nCells, total, keyB.p, G.cellStart.p);
        CHECK_LAUNCH();
        hipLaunchKernelGGL(k_grid_items, dim3(grid_for(total, SAMPLER_BUILD_GRID_CAP)), dim3(256), 0, s, total, keyB.p, G.items.p);
        CHECK_LAUNCH();
        std::vector<int32_t> hStart((size_t)nCells + 1);
        G.cellStart.download(hStart.data(), hStart.size(), s);      // (synchronises: the keys may go)
        for (int64_t q = 0; q < nCells; ++q) G.maxPop = std::max<int64_t>(G.maxPop, hStart[(size_t)q + 1] - hStart[(size_t)q]);
    } else {
        G.cellStart.zero(s);
        MFH_HIP(hipStreamSynchronize(s));
    }
    G.valid = true;
    G.buildMs = now_ms() - t0;
}

} // namespace

}} // namespace mfh::k

namespace mfhi {

void sampler_drop(mfh_ctx *c) {
    c->sampler.elem.reset();
    c->sampler.bdry.reset();
    c->sampler.bdryVerts.release();
    c->sampler.bdryParent.release();
}

} // namespace mfhi

namespace {

using namespace mfhi;
using mfh::k::grid_for;

// the contexts the sampler serves: a mesh of its own (not a matrix from triplets), all rows owned, a device
void require_sampler_context(mfh_ctx *c) {
    require(c != nullptr, MFH_ERR_INVALID, "null context");
    require(c->haveMesh && !c->external, MFH_ERR_STATE, "the field sampler needs a mesh (mfh_mesh_build / mfh_mesh_set)");
    require(c->mesh.nOwned == c->mesh.nNode, MFH_ERR_UNSUPPORTED,
            "the field sampler needs all rows owned: a row-partitioned context holds only this rank's part of the mesh");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
}

void mesh_box(const mfh_ctx *c, double *mn, double *mx, double &diag) {
    const HostMesh &m = c->mesh;
    for (int a = 0; a < m.dim; ++a) { mn[a] = m.vertPos[(size_t)a]; mx[a] = mn[a]; }
    for (int64_t v = 1; v < m.nVert; ++v)
        for (int a = 0; a < m.dim; ++a) { const double x = m.vertPos[(size_t)v * m.dim + a]; mn[a] = std::min(mn[a], x); mx[a] = std::max(mx[a], x); }
    diag = 0;
    for (int a = 0; a < m.dim; ++a) diag += (mx[a] - mn[a]) * (mx[a] - mn[a]);
    diag = std::sqrt(diag);
}

void ensure_element_grid(mfh_ctx *c) {
    if (c->sampler.elem.valid) return;
    const HostMesh &m = c->mesh;
    const double t0 = now_ms();
    double diag;
    mesh_box(c, c->sampler.bbMin, c->sampler.bbMax, diag);      // (kept for the boundary grid)
    c->sampler.pad = 1e-9 * diag;
    const double boxMs = now_ms() - t0;
    mfh::k::build_grid(c, c->sampler.elem, m.nElem, c->dElemNodes.p, m.elemNodes.data(), m.npe, m.dim + 1, c->sampler.bbMin, c->sampler.bbMax, c->sampler.pad);
    c->sampler.elem.hostMs += boxMs;
    c->sampler.elem.buildMs += boxMs;
}

// the boundary elements the mesh reports (mfh_mesh_get_boundary_elem_nodes / _parents); a mesh from mfh_mesh_set has none
void ensure_boundary_grid(mfh_ctx *c) {
    if (c->sampler.bdry.valid) return;
    const HostMesh &m = c->mesh;
    const int64_t nBE = m.nBE();
    std::vector<int32_t> verts((size_t)nBE * m.dim);
    for (int64_t b = 0; b < nBE; ++b)
        for (int k2 = 0; k2 < m.dim; ++k2) verts[(size_t)b * m.dim + k2] = m.bdryElemNodes[(size_t)b * m.npbe + k2];
    c->sampler.bdryVerts.upload(verts, c->stream);
    c->sampler.bdryParent.upload(m.bdryParent.data(), (size_t)nBE, c->stream);
    mfh::k::build_grid(c, c->sampler.bdry, nBE, c->sampler.bdryVerts.p, verts.data(), m.dim, m.dim, c->sampler.bbMin, c->sampler.bbMax, c->sampler.pad);
}

// a caller's array as the kernels use it: its device pointer, or a device buffer uploaded from / downloaded to its host array. `needed`: the
// kernels want the array even when the caller passed NULL.
template <class T> struct DevArray {
    DBuf<T> buf;
    T *p = nullptr, *host = nullptr;
    DevArray(T *user, size_t n, bool onDevice, bool needed, bool input, hipStream_t s) {
        if (!user && !needed) return;
        if (user && onDevice) { p = user; return; }
        buf.alloc(std::max<size_t>(n, 1));
        p = buf.p;
        if (user && input && n) MFH_HIP(hipMemcpyAsync(p, user, n * sizeof(T), hipMemcpyHostToDevice, s));
        if (user && !input) host = user;
    }
    void finish(hipStream_t s) { if (host && buf.n) buf.download(host, buf.n, s); }
};

// (element, barycentric coordinates[, closest point, squared distance]) of nP device points; any of bary / closest / sqDist may be null
void locate_device(mfh_ctx *c, int64_t nP, const double *dP, int32_t *elem, double *bary, double *closest, double *sqDist) {
    if (nP == 0) return;
    using namespace mfh::k;
    const HostMesh &m = c->mesh;
    ensure_element_grid(c);
    DBuf<uint8_t> flag;
    DBuf<int> any;
    flag.alloc((size_t)nP);
    any.alloc(1);
    any.zero(c->stream);
    const int grid = grid_for(nP, SAMPLER_POINT_GRID_CAP);
    const GridDesc g = grid_desc(c->sampler.elem);
    with_dim23(m.dim, [&](auto D) {
        launch_k(k_locate<D()>, dim3(grid), dim3(256), 0, c->stream, nP, dP, g, c->dElemNodes.p, m.npe, c->dVertPos.p, c->dGeo.p, c->geoStride, elem, bary,
                 closest, sqDist, flag.p, any.p);
    });
    CHECK_LAUNCH();
    int someOutside = 0;
    any.download(&someOutside, 1, c->stream);
    if (!someOutside) return;
    ensure_boundary_grid(c);
    if (c->sampler.bdry.nItems == 0) return;
    const GridDesc gb = grid_desc(c->sampler.bdry);
    with_dim23(m.dim, [&](auto D) {
        launch_k(k_closest_boundary<D()>, dim3(grid), dim3(256), 0, c->stream, nP, dP, flag.p, gb, c->sampler.bdryVerts.p, c->sampler.bdryParent.p,
                 c->dElemNodes.p, m.npe, c->dVertPos.p, c->dGeo.p, c->geoStride, elem, bary, closest, sqDist);
    });
    CHECK_LAUNCH();
}

void fill_grid_info(const mfh_ctx::SamplerGrid &G, mfh_sampler_grid_info &o) {
    o.built = G.valid ? 1 : 0;
    for (int a = 0; a < 3; ++a) o.cells[a] = G.valid ? G.nc[a] : 0;
    o.items = G.valid ? G.nItems : 0;
    o.pairs = G.valid ? G.nPairs : 0;
    o.max_cell_population = G.valid ? G.maxPop : 0;
    o.build_ms = G.valid ? G.buildMs : 0.0;
    o.host_ms = G.valid ? G.hostMs : 0.0;
}

} // namespace

mfh_status mfh_sampler_build(mfh_ctx *c) {
    MFH_TRY(c)
    require_sampler_context(c);
    ensure_element_grid(c);
    MFH_CATCH(c)
}

mfh_status mfh_sampler_info(const mfh_ctx *c, mfh_sampler_stats *out) {
    if (!c || !out) return MFH_ERR_INVALID;
    if (!c->haveMesh || c->external) return MFH_ERR_STATE;
    fill_grid_info(c->sampler.elem, out->elements);
    fill_grid_info(c->sampler.bdry, out->boundary);
    return MFH_OK;
}

mfh_status mfh_locate(mfh_ctx *c, int64_t nP, const double *P, int32_t *elem, double *bary, double *closest, double *sqDist, int32_t onDevice) {
    MFH_TRY(c)
    require_sampler_context(c);
    require(nP >= 0 && (nP == 0 || P), MFH_ERR_INVALID, "mfh_locate: nP >= 0 and a point array expected");
    if (nP == 0) return MFH_OK;
    const size_t N = (size_t)nP, d = (size_t)c->mesh.dim;
    const bool dev = onDevice != 0;
    DevArray<double> pts(const_cast<double *>(P), N * d, dev, true, true, c->stream);
    DevArray<int32_t> e(elem, N, dev, true, false, c->stream);
    DevArray<double> b(bary, N * (d + 1), dev, false, false, c->stream), cl(closest, N * d, dev, false, false, c->stream), sq(sqDist, N, dev, false, false, c->stream);
    locate_device(c, nP, pts.p, e.p, b.p, cl.p, sq.p);
    e.finish(c->stream); b.finish(c->stream); cl.finish(c->stream); sq.finish(c->stream);
    MFH_HIP(hipStreamSynchronize(c->stream));
    MFH_CATCH(c)
}

mfh_status mfh_sample_field(mfh_ctx *c, int64_t nP, const double *P, int32_t kind, const double *field, int32_t nComp, double *out, int32_t onDevice) {
    MFH_TRY(c)
    require_sampler_context(c);
    require(kind == MFH_FIELD_PER_VERTEX || kind == MFH_FIELD_PER_ELEMENT || kind == MFH_FIELD_PER_NODE, MFH_ERR_INVALID,
            "kind: MFH_FIELD_PER_VERTEX, MFH_FIELD_PER_ELEMENT or MFH_FIELD_PER_NODE");
    require(nComp >= 1, MFH_ERR_INVALID, "nComp >= 1 expected");
    require(nP >= 0 && (nP == 0 || (P && field && out)), MFH_ERR_INVALID, "mfh_sample_field: null argument");
    if (nP == 0) return MFH_OK;
    using namespace mfh::k;
    const HostMesh &m = c->mesh;
    const size_t N = (size_t)nP, d = (size_t)m.dim;
    const int64_t rows = kind == MFH_FIELD_PER_VERTEX ? m.nVert : (kind == MFH_FIELD_PER_ELEMENT ? m.nElem : m.nNode);
    const bool dev = onDevice != 0;
    DevArray<double> pts(const_cast<double *>(P), N * d, dev, true, true, c->stream);
    DevArray<double> f(const_cast<double *>(field), (size_t)rows * nComp, dev, true, true, c->stream);
    DevArray<double> res(out, N * nComp, dev, true, false, c->stream);
    DBuf<int32_t> e;                  // (I, B) stay on the device between the two kernels
    DBuf<double> b;
    e.alloc(N); b.alloc(N * (d + 1));
    locate_device(c, nP, pts.p, e.p, b.p, nullptr, nullptr);
    const EdgeTable et = edge_table(m.dim);
    const int grid = grid_for(nP, SAMPLER_POINT_GRID_CAP);
    with_dim23_deg(m.dim, m.deg, [&](auto D, auto G) {
        launch_k(k_sample_field<D(), G()>, dim3(grid), dim3(256), 0, c->stream, nP, e.p, b.p, c->dElemNodes.p, et, (int)kind, f.p, (int)nComp,
                 res.p);
    });
    CHECK_LAUNCH();
    res.finish(c->stream);
    MFH_HIP(hipStreamSynchronize(c->stream));
    MFH_CATCH(c)
}

mfh_status mfh_closest_node(mfh_ctx *c, int64_t nP, const double *P, int32_t *node, double *sqDist, int32_t onDevice) {
    MFH_TRY(c)
    require_sampler_context(c);
    require(nP >= 0 && (nP == 0 || P), MFH_ERR_INVALID, "mfh_closest_node: nP >= 0 and a point array expected");
    if (nP == 0) return MFH_OK;
    using namespace mfh::k;
    const HostMesh &m = c->mesh;
    const size_t N = (size_t)nP, d = (size_t)m.dim;
    const bool dev = onDevice != 0;
    DevArray<double> pts(const_cast<double *>(P), N * d, dev, true, true, c->stream);
    DevArray<int32_t> nd(node, N, dev, false, false, c->stream);
    DevArray<double> sq(sqDist, N, dev, false, false, c->stream);
    DBuf<int32_t> e;
    DBuf<double> b;
    e.alloc(N); b.alloc(N * (d + 1));
    locate_device(c, nP, pts.p, e.p, b.p, nullptr, nullptr);
    const EdgeTable et = edge_table(m.dim);
    const int grid = grid_for(nP, SAMPLER_POINT_GRID_CAP);
    with_dim23_deg(m.dim, m.deg, [&](auto D, auto G) {
        launch_k(k_closest_node<D(), G()>, dim3(grid), dim3(256), 0, c->stream, nP, pts.p, e.p, b.p, c->dElemNodes.p, et, c->dVertPos.p, nd.p,
                 sq.p);
    });
    CHECK_LAUNCH();
    nd.finish(c->stream); sq.finish(c->stream);
    MFH_HIP(hipStreamSynchronize(c->stream));
    MFH_CATCH(c)
}
