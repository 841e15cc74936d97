// HIP kernels for gfx950 (MI355X, CDNA4): element embedding, per-element stiffness blocks,
// owner-computes (gather) and atomic (scatter) assembly into a tiled block-CSR, block-CSR SpMV, the
// matrix-free operators and the element-level post-processing / shape-derivative kernels (the solver-side
// kernels are in mfh_kernels_solver.hip).  All arithmetic is FP64 (the reference's Real = double,
// Types.hh:8); the path is HBM/LDS bound, so there is no MFMA here.
//
// Data layout of K values ("tiled BSR"): block slot s, component c (row-major in the dim x dim
// block) lives at vals[((s >> 6) * NB + c) * 64 + (s & 63)], NB = dim*dim. Consecutive lanes that
// own consecutive slots therefore read/write 512 contiguous bytes per component: every wave-wide
// load/store of K is a fully coalesced 8 B/lane access on both the assembly and the SpMV side.
#include "mfh_device.hh"
#include "mfh_dispatch.hh"

namespace mfh { namespace k {

// ------------------------------------------------------------------------------------------------
// One dim x dim block of the element stiffness matrix:
//   K_ij[c][d] = sum_q w_q sum_ab d_a phi_i(q) C_{acdb} d_b phi_j(q)      (LinearElasticity.hh:183-231)
// With grad phi_i(q) = alpha_i(q) u_a + beta_i(q) u_b the quadrature sum collapses onto the four
// precomputed pair coefficients S = vol * sum_q w_q {a_i a_j, a_i b_j, b_i a_j, b_i b_j}:
//   H[a][b] = sum_q w_q d_a phi_i d_b phi_j = u_a (S0 v_a + S1 v_b)^T + u_b (S2 v_a + S3 v_b)^T
// (same quadrature rule and points as the reference: GaussQuadrature.hh:115-127,283-295).
// ------------------------------------------------------------------------------------------------
// components per matrix entry: dim x dim blocks for elasticity, 1 for the scalar operators
template <int DIM, int MAT> DEV constexpr int mat_nb() { return (MAT == MAT_LAPLACE || MAT == MAT_MASS || MAT == MAT_MASS_RHO || MAT == MAT_GEOM) ? 1 : DIM * DIM; }

// material part of a block: K from H = sum_q w_q grad phi_i (x) grad phi_j and the element's tensor
// (sig: the element's prestress, MAT_GEOM only -- flattened, tensor shear entries; no other flavour reads it)
template <int DIM, int MAT>
DEV void block_from_H(const double *__restrict__ g, const double (&H)[DIM][DIM], double *K, const double *__restrict__ sig = nullptr);

// H from the (s,t) support offsets of the two nodes and the pair's four quadrature coefficients (one row of
// ShapeTables::pairTable): the table-driven form of the assembly kernel (quadratic elements)
template <int DIM>
DEV void pair_H(const double *__restrict__ g, uint32_t offs /* bytes: 3 DIM-offsets of s_i, t_i, s_j, t_j */, double S0, double S1, double S2,
                double S3, double (&H)[DIM][DIM]) {
    // MFH_ASM_ABLATE (timing-only builds of round 6, docs/design/04_2 (xiii): K comes out wrong): 1 = the loads that belong to the ROW node of a
    // contribution (its two support gradients, the volume, the Lame parameters) are replaced by values the lane already has -- what a row-lane
    // decomposition could save at most on the load side; 2 = no element record is read at all
#ifndef MFH_ASM_ABLATE
#define MFH_ASM_ABLATE 0
#endif
    const double vol = MFH_ASM_ABLATE >= 1 ? 1.0 : g[12];
    S0 *= vol; S1 *= vol; S2 *= vol; S3 *= vol;
    const char *gb = reinterpret_cast<const char *>(g);
    const double *gsi = reinterpret_cast<const double *>(gb + (offs & 0xffu)), *gti = reinterpret_cast<const double *>(gb + ((offs >> 8) & 0xffu)),
                 *gsj = reinterpret_cast<const double *>(gb + ((offs >> 16) & 0xffu)), *gtj = reinterpret_cast<const double *>(gb + (offs >> 24));
    double ua[DIM], ub[DIM], p[DIM], q[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        ua[a] = MFH_ASM_ABLATE >= 1 ? S0 + a : gsi[a]; ub[a] = MFH_ASM_ABLATE >= 1 ? S1 - a : gti[a];
        const double va = MFH_ASM_ABLATE >= 2 ? S2 + a : gsj[a], vb = MFH_ASM_ABLATE >= 2 ? S3 - a : gtj[a];
        p[a] = S0 * va + S1 * vb;
        q[a] = S2 * va + S3 * vb;
    }
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) H[a][b] = ua[a] * p[b] + ub[a] * q[b];
}

template <int DIM, int DEG, int MAT>
DEV void elem_block(const double *__restrict__ g, const double *__restrict__ pairTab, const PairConst &pc, int i, int j, double *K,
                    const double *__restrict__ sig = nullptr) {
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    const double vol = g[12];
    if (MAT == MAT_MASS || MAT == MAT_MASS_RHO) {
        // int phi_i phi_j = vol * (reference value): exact for straight-sided simplices, equal to the
        // reference's Quadrature<K, 2 Deg> (exact for this integrand) up to rounding (MassMatrix.hh:66-77)
        K[0] = vol * pairTab[i * NPE + j];
        return;
    }
    double H[DIM][DIM];
    if (DEG == 1) {
        double gi[DIM], gj[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) { gi[a] = g[i * DIM + a]; gj[a] = g[j * DIM + a] * vol; }
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int b = 0; b < DIM; ++b) H[a][b] = gi[a] * gj[b];
    } else {
        const int si = sup_s<DIM, DEG>(i), ti = sup_t<DIM, DEG>(i), sj = sup_s<DIM, DEG>(j), tj = sup_t<DIM, DEG>(j);
        // Pair coefficients S = sum_q w_q coef_i(q) coef_j(q). Node i has the terms
        //   A: (4 lambda_l - o) grad lambda_{s_i}, l = s_i, o = 1 (vertex node) | l = t_i, o = 0 (edge node)
        //   B: (4 lambda_{s_i})  grad lambda_{t_i}, edge nodes only
        // and sum_q w_q (4 l_a - o)(4 l_b - o') takes only six values with the reference's rule (by
        // (o, o') class and a == b / a != b). They are read from the host-built quadrature table
        // (build_shape_tables), so no per-lane table loads are needed.
        constexpr int NV = DIM + 1;
        const bool vi = i < NV, vj = j < NV;
        const int lAi = vi ? si : ti, lBi = si, lAj = vj ? sj : tj, lBj = sj;
        // closed form of the table: S = c1 + [a==b] c2 - c3 (o + o') + o o'  with c1 = 16 m_ab (a != b),
        // c2 = 16 (m_aa - m_ab), c3 = 4 m_a (all three from the reference's quadrature rule). Pure
        // arithmetic on purpose: select chains over named constants get turned into a scratch table.
        const double c1 = pc.ee_ne, c2 = pc.ee_eq - pc.ee_ne, c3 = pc.ee_ne - pc.ve_ne;
        const double oi = vi ? 1.0 : 0.0, oj = vj ? 1.0 : 0.0;
        auto coef = [&](bool eq, double o, double o2) -> double { return (c1 + (eq ? c2 : 0.0)) - c3 * (o + o2) + o * o2; };
        double S0 = coef(lAi == lAj, oi, oj);                                    // A_i A_j
        double S1 = vj ? 0.0 : coef(lAi == lBj, oi, 0.0);                        // A_i B_j
        double S2 = vi ? 0.0 : coef(lBi == lAj, 0.0, oj);                        // B_i A_j
        double S3 = (vi | vj) ? 0.0 : coef(lBi == lBj, 0.0, 0.0);                // B_i B_j
        S0 *= vol; S1 *= vol; S2 *= vol; S3 *= vol;
        double ua[DIM], ub[DIM], p[DIM], q[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            ua[a] = g[si * DIM + a]; ub[a] = g[ti * DIM + a];
            const double va = g[sj * DIM + a], vb = g[tj * DIM + a];
            p[a] = S0 * va + S1 * vb;
            q[a] = S2 * va + S3 * vb;
        }
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int b = 0; b < DIM; ++b) H[a][b] = ua[a] * p[b] + ub[a] * q[b];
    }
    block_from_H<DIM, MAT>(g, H, K, sig);
}

template <int DIM, int MAT>
DEV void block_from_H(const double *__restrict__ g, const double (&H)[DIM][DIM], double *K, const double *__restrict__ sig) {
    if (MAT == MAT_GEOM) {
        // geometric stiffness: int grad phi_i . sigma_e grad phi_j = H : sigma_e (sigma constant on the element; sigma = I is MAT_LAPLACE)
        constexpr int FL = DIM * (DIM + 1) / 2;
        double sg[FL];
#pragma unroll
        for (int q = 0; q < FL; ++q) sg[q] = sig[q];
        double v = 0;
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int b = 0; b < DIM; ++b) v += H[a][b] * sg[flat_idx<DIM>(a, b)];
        K[0] = v;
    } else if (MAT == MAT_LAPLACE) {
        // int grad phi_i . grad phi_j = tr(H)   (Laplacian.hh:38-48; Poisson.hh:33-38)
        double tr = 0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) tr += H[a][a];
        K[0] = tr;
    } else if (MAT == MAT_ISO) {
        // C_acdb = lambda d_ac d_db + mu (d_ad d_cb + d_ab d_cd)  =>  K = lambda H + mu H^T + mu tr(H) I
#if defined(MFH_ASM_ABLATE) && MFH_ASM_ABLATE >= 1
        const double lam = H[0][0], mu = H[1][1];      // (timing-only build: no load of the Lame parameters)
#else
        const double lam = g[13], mu = g[14];
#endif
        double tr = 0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) tr += H[a][a];
#pragma unroll
        for (int c = 0; c < DIM; ++c)
#pragma unroll
            for (int d = 0; d < DIM; ++d) K[c * DIM + d] = lam * H[c][d] + mu * H[d][c] + (c == d ? mu * tr : 0.0);
    } else if (MAT == MAT_ORTHO) {
        // orthotropic D in its material axes: C_aadd = N[a][d], C_acac = C_acca = S(a,c) (a != c), every other entry 0
        //   K[c][c] = N[c][c] H[c][c] + sum_{a != c} S(a,c) H[a][a] ;   K[c][d] = N[c][d] H[c][d] + S(c,d) H[d][c]   (c != d)
#pragma unroll
        for (int c = 0; c < DIM; ++c)
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                double v = g[13 + npack<DIM>(c, d)] * H[c][d];
                if (c == d) {
#pragma unroll
                    for (int a = 0; a < DIM; ++a)
                        if (a != c) v += g[ortho_shear_offset<DIM>() + flat_idx<DIM>(a, c) - DIM] * H[a][a];
                } else v += g[ortho_shear_offset<DIM>() + flat_idx<DIM>(c, d) - DIM] * H[d][c];
                K[c * DIM + d] = v;
            }
    } else {
        // C_acdb = D(flat(a,c), flat(d,b))      (ElasticityTensor.hh:274-277)
        constexpr int ND = (DIM * (DIM + 1) / 2) * (DIM * (DIM + 1) / 2 + 1) / 2;
        double D[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) D[k] = g[13 + k];
#pragma unroll
        for (int c = 0; c < DIM; ++c)
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                double acc = 0;
#pragma unroll
                for (int a = 0; a < DIM; ++a)
#pragma unroll
                    for (int b = 0; b < DIM; ++b) acc += H[a][b] * D[dpack<DIM>(flat_idx<DIM>(a, c), flat_idx<DIM>(d, b))];
                K[c * DIM + d] = acc;
            }
    }
}

// ------------------------------------------------------------------------------------------------
// K1: element embedding + material record     (EmbeddedElement.hh:162-241, ElasticityTensor.hh:100-164)
// matMode: 0 const (lambda,mu) | 1 iso field (E[],nu[]) | 2 const general D (packed upper) | 5 const orthotropic-pattern D |
//          3 orthotropic field (9 / 4 params per element) | 4 tensor field (flatLen^2 per element)
// ------------------------------------------------------------------------------------------------
// signed volume and barycentric gradients of a simplex from its corner positions (EmbeddedElement.hh:182-189 triangle,
// :223-230 tet): gl[k] = grad lambda_k
template <int DIM>
DEV void embed_simplex(const double (&P)[DIM + 1][DIM], double (&gl)[DIM + 1][DIM], double &vol) {
    if (DIM == 3) {
        // n0 = (p3-p1)x(p2-p1); 6V = (p0-p1).n0; gl0 = n0/6V; gl1 = (p2-p0)x(p3-p0)/6V; ...   (:223-230)
        auto cross = [](const double *a, const double *b, double *o) {
            o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
        };
        double d31[3], d21[3], d01[3], d20[3], d30[3], d10[3], n[4][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            d31[a] = P[3][a] - P[1][a]; d21[a] = P[2][a] - P[1][a]; d01[a] = P[0][a] - P[1][a];
            d20[a] = P[2][a] - P[0][a]; d30[a] = P[3][a] - P[0][a]; d10[a] = P[1][a] - P[0][a];
        }
        cross(d31, d21, n[0]); cross(d20, d30, n[1]); cross(d30, d10, n[2]); cross(d10, d20, n[3]);
        const double vol6 = d01[0] * n[0][0] + d01[1] * n[0][1] + d01[2] * n[0][2];
        vol = vol6 / 6.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a) gl[k][a] = n[k][a] / vol6;
    } else {
        // e0=p2-p1, e1=p0-p2, e2=p1-p0; 2A = e1.x e2.y - e1.y e2.x; gl_k = (-e_k.y, e_k.x)/2A   (:182-189)
        double E[3][2];
#pragma unroll
        for (int a = 0; a < 2; ++a) { E[0][a] = P[2][a] - P[1][a]; E[1][a] = P[0][a] - P[2][a]; E[2][a] = P[1][a] - P[0][a]; }
        const double dA = E[1][0] * E[2][1] - E[1][1] * E[2][0];
        vol = dA / 2.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { gl[k][0] = -E[k][1] / dA; gl[k][1] = E[k][0] / dA; }
    }
}

template <int DIM>
__global__ void __launch_bounds__(256) k_geometry(int64_t nElem, const int32_t *__restrict__ elemNodes, int npe,
                                                  const double *__restrict__ vertPos, const double *__restrict__ mp,
                                                  int matMode, double *__restrict__ geo, int stride, int *negCount) {
    // The records are built in LDS (row stride + 1 doubles: lanes on different banks) and copied out as whole contiguous lines:
    // written by their own lanes they would go out in 8-byte pieces at a stride of 128+ bytes (0.29 -> 0.2 ms at config 3).
    extern __shared__ __attribute__((aligned(16))) double recs[];   // [256][stride + 1]
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double *g = recs + (size_t)threadIdx.x * (stride + 1);
    for (int k = 0; k < stride; ++k) g[k] = 0.0;
    if (e < nElem) {
    double P[DIM + 1][DIM];
#pragma unroll
    for (int k = 0; k <= DIM; ++k) {
        const int64_t v = elemNodes[e * npe + k];
#pragma unroll
        for (int a = 0; a < DIM; ++a) P[k][a] = vertPos[v * DIM + a];
    }
    double vol, gl[DIM + 1][DIM];
    embed_simplex<DIM>(P, gl, vol);
#pragma unroll
    for (int k = 0; k <= DIM; ++k)
#pragma unroll
        for (int a = 0; a < DIM; ++a) g[k * DIM + a] = gl[k][a];
    if (DIM == 2) {
#pragma unroll
        for (int k = 6; k < 12; ++k) g[k] = 0.0;
    }
    g[12] = vol;
    if (!(vol >= 0)) atomicAdd(negCount, 1);
    constexpr int FL = DIM * (DIM + 1) / 2;
    constexpr int ND = FL * (FL + 1) / 2;
    if (matMode == 0) { g[13] = mp[0]; g[14] = mp[1]; }
    else if (matMode == 1) {
        const double E = mp[e], nu = mp[nElem + e];
        // positive definite iff E > 0 and -1 < nu < 1/2 (3D) or -1 < nu < 1 (2D plane stress)
        if (!(E > 0 && nu > -1.0 && nu < (DIM == 3 ? 0.5 : 1.0))) atomicAdd(negCount + 1, 1);
        double lam = (nu * E) / ((1.0 + nu) * (1.0 - 2.0 * nu));
        if (DIM == 2) lam = (nu * E) / (1.0 - nu * nu);     // plane stress (ElasticityTensor.hh:108-112)
        g[13] = lam; g[14] = E / (2.0 + 2.0 * nu);
    } else if (matMode == 2) {
        for (int k = 0; k < ND; ++k) g[13 + k] = mp[k];
    } else if (matMode == 5) {
        for (int k = 0; k < DIM * (DIM + 1) / 2 + FL - DIM; ++k) g[13 + k] = mp[k];   // constant tensor with the orthotropic pattern
    } else if (matMode == 3) {
        // compact orthotropic record (MAT_ORTHO): normal block + shear stiffnesses, see npack / ortho_shear_offset
        if (DIM == 3) {
            const double *q = mp + e * 9;   // Ex,Ey,Ez,nuYX,nuZX,nuZY,muYZ,muZX,muXY  (:136-152)
            const double a00 = 1.0 / q[0], a01 = -q[3] / q[1], a02 = -q[4] / q[2], a11 = 1.0 / q[1], a12 = -q[5] / q[2],
                         a22 = 1.0 / q[2];
            const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
            const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
            const double det = a00 * c00 + a01 * c01 + a02 * c02;
            // Sylvester on the compliance block + positive shear moduli: otherwise the tensor is indefinite (negCount[1])
            if (!(a00 > 0 && c22 > 0 && det > 0 && q[6] > 0 && q[7] > 0 && q[8] > 0)) atomicAdd(negCount + 1, 1);
            g[13 + npack<3>(0, 0)] = c00 / det; g[13 + npack<3>(0, 1)] = c01 / det; g[13 + npack<3>(0, 2)] = c02 / det;
            g[13 + npack<3>(1, 1)] = c11 / det; g[13 + npack<3>(1, 2)] = c12 / det; g[13 + npack<3>(2, 2)] = c22 / det;
            g[ortho_shear_offset<3>() + 0] = q[6]; g[ortho_shear_offset<3>() + 1] = q[7]; g[ortho_shear_offset<3>() + 2] = q[8];
        } else {
            const double *q = mp + e * 4;   // Ex,Ey,nuYX,muXY                          (:154-164)
            const double a00 = 1.0 / q[0], a01 = -q[2] / q[1], a11 = 1.0 / q[1];
            const double det = a00 * a11 - a01 * a01;
            if (!(a00 > 0 && det > 0 && q[3] > 0)) atomicAdd(negCount + 1, 1);
            g[13 + npack<2>(0, 0)] = a11 / det; g[13 + npack<2>(0, 1)] = -a01 / det; g[13 + npack<2>(1, 1)] = a00 / det;
            g[ortho_shear_offset<2>()] = q[3];
        }
    } else {
        const double *q = mp + e * FL * FL;
        for (int r = 0; r < FL; ++r)
            for (int c = r; c < FL; ++c) g[13 + dpack<DIM>(r, c)] = q[r * FL + c];
    }
    }
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * blockDim.x;
    const int nLive = (int)(nElem - e0 < (int64_t)blockDim.x ? nElem - e0 : (int64_t)blockDim.x);
    double *out = geo + e0 * stride;
    for (int q = threadIdx.x; q < nLive * stride; q += blockDim.x) {
        const int el = q / stride;
        out[q] = recs[(size_t)el * (stride + 1) + (q - el * stride)];
    }
}

// ------------------------------------------------------------------------------------------------
// K2+K3+K4 fused, owner-computes: one workgroup per row chunk (<= chunkSlots blocks of consecutive
// block rows). Every (element, i, j) contribution to those rows is computed by one lane and
// accumulated in LDS with ds_add_f64; the finished rows are written once, coalesced, with plain
// stores. No global atomics, no read-modify-write of K, no zero-fill pass.
// ------------------------------------------------------------------------------------------------
// isotropic / scalar flavours: 8 waves per SIMD (64 VGPRs; 69 without the hint) so that the registers allow the 8 workgroups
// per CU that the 18 KB of LDS accumulators do (measured 5.42 vs 5.67 ms at config 3 on one box)
// UPPER only names the instantiation (profiles tell the launches on the upper-triangle storage from those on the full one):
// which blocks exist is decided by the gather lists, the code is the same.
// Gather lists in PACKED form (a.chunkElemBase != null): code = (element - chunkElemBase[chunk]) << 7 | (i NPE + j) -- a shift and a
// mask instead of two divisions, and no 2^32 / NPE^2 ceiling on the element count. Quadratic elements read the pair's four quadrature
// coefficients and the byte offsets of its four barycentric gradients from a table in LDS (one row of ShapeTables::pairTable per
// (i, j): built by the workgroup from 3.2 KB of L2-resident data) instead of re-deriving them per contribution from the node
// indices (support-vertex lookups, vertex / edge selects, the closed form of the coefficients: ~50 of the 141 VALU instructions
// per contribution of the round-2 kernel).
template <int DIM, int DEG, int MAT> DEV constexpr bool asm_uses_table() { return DEG == 2 && MAT != MAT_MASS && MAT != MAT_MASS_RHO; }
constexpr int ASM_CODE_SHIFT = 7;

template <int DIM, int DEG, int MAT, bool UPPER = false, bool DET = false>
__global__ void __launch_bounds__(256, (MAT == MAT_GENERAL || MAT == MAT_ORTHO) ? 1 : 8) k_assemble_gather(AsmArgs a) {
    constexpr int NB = mat_nb<DIM, MAT>();
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr bool TAB = asm_uses_table<DIM, DEG, MAT>();
    extern __shared__ __attribute__((aligned(16))) double acc[];   // [NB][chunkSlots + 2] (+ pair table [NPE^2][4] doubles + [NPE^2] u32)
    const int CS = a.chunkSlots + 2;
    double *tabS = acc + (size_t)NB * CS;
    uint32_t *tabO = reinterpret_cast<uint32_t *>(tabS + NPE * NPE * 4);
    uint32_t *turn = tabO + NPE * NPE;                                 // DET: whose turn it is to add (see below); the launcher sizes the LDS for it
    const PairConst pc{a.pairConst[0], a.pairConst[1], a.pairConst[2], a.pairConst[3], a.pairConst[4], a.pairConst[5]};
    const int64_t item = a.xcd == 1 ? xcd_item(blockIdx.x, gridDim.x) : (a.xcd > 1 ? xcd_group_item(blockIdx.x, gridDim.x, a.xcd) : (int64_t)blockIdx.x);
    const int64_t chunk = a.chunkOrder ? (int64_t)a.chunkOrder[item] : item;
    const int r0 = a.chunkRow[chunk], r1 = a.chunkRow[chunk + 1];
    const int s0 = a.rowPtr[r0];
    const int ns = a.rowPtr[r1] - s0;
    const uint32_t eBase = a.chunkElemBase ? (uint32_t)a.chunkElemBase[chunk] : 0u;
    // LDS index = local slot + (s0 & 1): LDS pairs (2p, 2p+1) then coincide with 16-byte aligned
    // pairs of the tiled global layout and the write-out can use dwordx4 stores
    const int par = s0 & 1;
    for (int t = threadIdx.x; t < ns + par; t += 256)
#pragma unroll
        for (int c = 0; c < NB; ++c) acc[c * CS + t] = 0.0;
    if (DET && threadIdx.x == 0) *turn = 0u;
    if (TAB) {
        for (int t = threadIdx.x; t < NPE * NPE; t += 256) {
            const int i = t / NPE, j = t - i * NPE;
#pragma unroll
            for (int k = 0; k < 4; ++k) tabS[t * 4 + k] = a.pairTable[t * 4 + k];
            tabO[t] = (uint32_t)(sup_s<DIM, DEG>(i) * DIM * 8) | ((uint32_t)(sup_t<DIM, DEG>(i) * DIM * 8) << 8) |
                      ((uint32_t)(sup_s<DIM, DEG>(j) * DIM * 8) << 16) | ((uint32_t)(sup_t<DIM, DEG>(j) * DIM * 8) << 24);
        }
    }
    __syncthreads();
    const int64_t kb = a.contribPtr[chunk], ke = a.contribPtr[chunk + 1];
    // U independent contributions per lane and trip: their index loads, element-record loads and
    // block arithmetic have no mutual dependence, so the loads of all U are in flight together
    // (the kernel is latency-bound: rocprof shows 65 % of wave cycles in s_waitcnt at U = 1).
    // Option "deterministic" (template parameter DET, chosen by the launcher from a.det): the four waves of the workgroup add their contributions to the LDS accumulators one wave after the
    // other, trip by trip, so that the contributions of a slot always meet in the same order (inside one wave the lanes of an LDS atomic are
    // applied in a fixed order; between waves the order is a matter of timing, and the last bits of K with it). Every lane runs the same
    // number of trips. The turns are handed on through a token in LDS -- the wave whose (trip, u, wave) number the token shows adds, makes
    // its adds visible and increments the token -- instead of a workgroup barrier per turn (round 4: eight barriers per trip, kernel 1.15x
    // the default): only the wave that is next waits, the others go on fetching and computing their next contribution.
    constexpr int U = 2;
    constexpr bool det = DET;          // a template parameter: the default instantiations carry no barrier inside the loop
    unsigned turnNo = threadIdx.x >> 6;                                // this wave's next turn: (trip U + u) 4 + wave
    for (int64_t k0 = kb + threadIdx.x; det ? (k0 - threadIdx.x < ke) : (k0 < ke); k0 += 256 * U) {
        uint32_t code[U];
        int ls[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t kk = k0 + (int64_t)u * 256;
            ok[u] = kk < ke;
            code[u] = ok[u] ? a.contribCode[kk] : a.contribCode[kb];
            ls[u] = (ok[u] ? (int)a.contribSlot[kk] : 0) + par;
        }
        // the element records are fetched one contribution after the other (sched_barrier): a record is 30+ VGPRs of loads in
        // flight, and two at a time cost more in occupancy than they hide in latency (iso P2: 99 VGPRs / 5 waves per SIMD
        // 6.4 ms against 64 VGPRs / 8 waves 5.1 ms; the anisotropic flavours drop from 168 / 129 to 100 / 80 VGPRs)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double K[NB];
            // Lanes past the end of the chunk's list skip the block arithmetic, and a wave none of whose lanes has a contribution left
            // skips it altogether (round 5; before, they computed a dummy block: with ~655 contributions per chunk and trips of 512 that
            // was a fifth of the executed block evaluations and record fetches).
            if (ok[u]) {
            uint32_t e;
            int ij;
            if (a.chunkElemBase) { e = eBase + (code[u] >> ASM_CODE_SHIFT); ij = (int)(code[u] & ((1u << ASM_CODE_SHIFT) - 1)); }
            else { e = code[u] / (NPE * NPE); ij = (int)(code[u] - e * (NPE * NPE)); }
            const double *g = a.geo + (int64_t)e * a.geoStride;
            if (TAB) {
                typedef double dv2 __attribute__((ext_vector_type(2)));
                const dv2 s01 = *reinterpret_cast<const dv2 *>(&tabS[ij * 4]), s23 = *reinterpret_cast<const dv2 *>(&tabS[ij * 4 + 2]);
                const uint32_t offs = tabO[ij];
                double H[DIM][DIM];
                pair_H<DIM>(g, offs, s01.x, s01.y, s23.x, s23.y, H);
                if (MAT == MAT_GEOM) block_from_H<DIM, MAT>(g, H, K, a.sigma + (int64_t)e * (DIM * (DIM + 1) / 2));   // the context's prestress (mfh_set_prestress)
                else block_from_H<DIM, MAT>(g, H, K);
            } else {
                const int i = ij / NPE, j = ij - i * NPE;
                if (MAT == MAT_GEOM) elem_block<DIM, DEG, MAT>(g, a.pairTable, pc, i, j, K, a.sigma + (int64_t)e * (DIM * (DIM + 1) / 2));
                else elem_block<DIM, DEG, MAT>(g, (MAT == MAT_MASS || MAT == MAT_MASS_RHO) ? a.massTable : a.pairTable, pc, i, j, K);
                if (MAT == MAT_MASS_RHO) K[0] *= a.density[e];     // the context's density field (mfh_set_density): rho_e vol_e m_ij
            }
            }
            if (det) {
                if ((threadIdx.x & 63) == 0)
                    while (__hip_atomic_load(turn, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != turnNo) __builtin_amdgcn_s_sleep(1);
                if (ok[u]) {
#pragma unroll
                    for (int c = 0; c < NB; ++c) unsafeAtomicAdd(&acc[c * CS + ls[u]], K[c]);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");          // the adds are performed before the token moves on
                if ((threadIdx.x & 63) == 0) __hip_atomic_store(turn, turnNo + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                turnNo += 4u;
            } else if (ok[u]) {
#pragma unroll
                for (int c = 0; c < NB; ++c) unsafeAtomicAdd(&acc[c * CS + ls[u]], K[c]);
                // (round 6, measured and removed: even / odd lanes walking the 9 components in opposite orders, or three rotations by lane % 3, so that lanes adding
                // to the SAME slot do not meet at one address -- 3.10 -> 3.32 / 3.55 ms: a ds_add_f64 costs per INSTRUCTION, not per active lane, docs/design/04_2 (xiii))
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();
    // write-out: one 16-byte store per lane and component (two adjacent slots); the store path is
    // issue-bound, so halving the store-instruction count matters more than anything else here
    const int nl = ns + par;                               // LDS entries [par, nl) are live
    const int64_t sbase = (int64_t)s0 - par;               // even: LDS index t <-> global slot sbase + t
    const int pfirst = par;                                // first fully live pair (pair 0 holds a dead entry if par)
    const int plast = nl >> 1;                             // pairs [pfirst, plast) are fully live
    for (int p = pfirst + threadIdx.x; p < plast; p += 256) {
        const int t = 2 * p;
        const int64_t s = sbase + t;
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            const double2 v = *reinterpret_cast<const double2 *>(&acc[c * CS + t]);
            double2 *dst = reinterpret_cast<double2 *>(&a.vals[tiled_index(s, c, NB)]);
            typedef double dv2 __attribute__((ext_vector_type(2)));
            // non-temporal: K is not re-read by this kernel; keeping it out of L2 leaves the cache to the
            // element records and gather lists (2.12 -> 1.71 ms at 1.5 M P2 tets)
            dv2 w = {v.x, v.y};
            __builtin_nontemporal_store(w, reinterpret_cast<dv2 *>(dst));
        }
    }
    // the (at most two) slots that are not part of a fully live pair
    if (threadIdx.x < 2) {
        const int t = threadIdx.x == 0 ? 1 : nl - 1;       // LDS entry 1 (if par) / last entry (if nl odd)
        const bool live = threadIdx.x == 0 ? (par == 1 && nl > 1) : ((nl & 1) && nl - 1 >= par && !(par == 1 && nl - 1 == 1));
        if (live) {
            const int64_t s = sbase + t;
#pragma unroll
            for (int c = 0; c < NB; ++c) a.vals[tiled_index(s, c, NB)] = acc[c * CS + t];
        }
    }
}

// key of a row chunk for the launch order: the element of its median contribution (the lists are element-major inside a chunk)
__global__ void __launch_bounds__(256) k_chunk_keys(int64_t nChunk, const int64_t *__restrict__ contribPtr, const uint32_t *__restrict__ contribCode,
                                                    const int32_t *__restrict__ chunkElemBase, uint32_t npe2, uint32_t *__restrict__ keys) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nChunk) return;
    const int64_t kb = contribPtr[b], ke = contribPtr[b + 1];
    if (ke <= kb) { keys[b] = 0xffffffffu; return; }
    const uint32_t c = contribCode[kb + (ke - kb) / 2];
    keys[b] = chunkElemBase ? (uint32_t)chunkElemBase[b] + (c >> ASM_CODE_SHIFT) : c / npe2;
}

// absolute codes e NPE^2 + ij -> packed chunk-relative codes (see k_assemble_gather); one wave per chunk. Pass 1 (rewrite == 0) finds
// the smallest element of every chunk and raises flag[0] when a chunk's elements span 2^25 or more (the packed element field is 25
// bits wide); pass 2 rewrites the codes in place.
__global__ void __launch_bounds__(64) k_pack_codes(int64_t nChunk, const int64_t *__restrict__ contribPtr, uint32_t *__restrict__ contribCode,
                                                   uint32_t npe2, int32_t *__restrict__ chunkElemBase, int *flag, int rewrite) {
    const int64_t b = blockIdx.x;
    const int64_t kb = contribPtr[b], ke = contribPtr[b + 1];
    if (rewrite) {
        const uint32_t lo = (uint32_t)chunkElemBase[b];
        for (int64_t k = kb + threadIdx.x; k < ke; k += 64) {
            const uint32_t c = contribCode[k], e = c / npe2;
            contribCode[k] = ((e - lo) << ASM_CODE_SHIFT) | (c - e * npe2);
        }
        return;
    }
    uint32_t lo = 0xffffffffu, hi = 0;
    for (int64_t k = kb + threadIdx.x; k < ke; k += 64) {
        const uint32_t e = contribCode[k] / npe2;
        lo = e < lo ? e : lo;
        hi = e > hi ? e : hi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if (ke <= kb) lo = 0;
    if (threadIdx.x == 0) {
        chunkElemBase[b] = (int32_t)lo;
        if (ke > kb && hi - lo >= (1u << (32 - ASM_CODE_SHIFT))) atomicExch(flag, 1);
    }
}

// Baseline variant: element-major, one lane per (element,i,j) block, global_atomic_add_f64 scatter
// into the (pre-zeroed) tiled values through the element->slot scatter map.
template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_assemble_atomic(AsmArgs a) {
    constexpr int NB = mat_nb<DIM, MAT>();
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    const PairConst pc{a.pairConst[0], a.pairConst[1], a.pairConst[2], a.pairConst[3], a.pairConst[4], a.pairConst[5]};
    const int64_t total = a.nElem * (NPE * NPE);
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
        const int32_t slot = a.scatterSlot[k];
        if (slot < 0) continue;
        const int64_t e = k / (NPE * NPE);
        const int ij = (int)(k - e * (NPE * NPE));
        const int i = ij / NPE, j = ij - i * NPE;
        double K[NB];
        elem_block<DIM, DEG, MAT>(a.geo + e * a.geoStride, MAT == MAT_MASS ? a.massTable : a.pairTable, pc, i, j, K);
#pragma unroll
        for (int c = 0; c < NB; ++c) unsafeAtomicAdd(&a.vals[tiled_index(slot, c, NB)], K[c]);
    }
}

// Dense per-element Ke (parity/debug): full (NPE*DIM)^2 row-major.
template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_element_stiffness(AsmArgs a, int64_t first, int64_t count, double *out) {
    constexpr int NB = mat_nb<DIM, MAT>();
    constexpr int BS = NB == 1 ? 1 : DIM;          // block edge
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr int KS = NPE * BS;
    const PairConst pc{a.pairConst[0], a.pairConst[1], a.pairConst[2], a.pairConst[3], a.pairConst[4], a.pairConst[5]};
    const int64_t total = count * (NPE * NPE);
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
        const int64_t el = k / (NPE * NPE);
        const int ij = (int)(k - el * (NPE * NPE));
        const int i = ij / NPE, j = ij - i * NPE;
        double K[NB];
        elem_block<DIM, DEG, MAT>(a.geo + (first + el) * a.geoStride, MAT == MAT_MASS ? a.massTable : a.pairTable, pc, i, j, K);
        double *o = out + el * KS * KS;
#pragma unroll
        for (int c = 0; c < BS; ++c)
#pragma unroll
            for (int d = 0; d < BS; ++d) o[(i * BS + c) * KS + j * BS + d] = K[c * BS + d];
    }
}

// Absolute row sums of the element matrices (mfh_explicit_dt, mfh_explicit.hip: the Gershgorin bound on M_L^-1 K): one lane per (element, local
// node i) walks the NPE blocks of row i with the arithmetic of the assembly (elem_block: the values K holds) and writes
// out[(e NPE + i) DIM + c] = sum_j sum_d |K_e[(i, c), (j, d)]|. Every entry is written once, j ascending: no atomics.
template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_elem_abs_rowsums(AsmArgs a, double *__restrict__ out) {
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    const PairConst pc{a.pairConst[0], a.pairConst[1], a.pairConst[2], a.pairConst[3], a.pairConst[4], a.pairConst[5]};
    const int64_t total = a.nElem * NPE;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
        const int64_t e = k / NPE;
        const int i = (int)(k - e * NPE);
        double rs[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) rs[c] = 0.0;
        for (int j = 0; j < NPE; ++j) {
            double K[DIM * DIM];
            elem_block<DIM, DEG, MAT>(a.geo + e * a.geoStride, a.pairTable, pc, i, j, K);
#pragma unroll
            for (int c = 0; c < DIM; ++c)
#pragma unroll
                for (int d = 0; d < DIM; ++d) rs[c] += fabs(K[c * DIM + d]);
        }
#pragma unroll
        for (int c = 0; c < DIM; ++c) out[k * DIM + c] = rs[c];
    }
}

// ------------------------------------------------------------------------------------------------
// K8: constantStrainLoad (LinearElasticity.hh:551-562, :135-162): l_i = (C_e : cstrain) . int grad phi_i,
// one lane per (element, node); int grad phi_i = vol (al_i gl[s_i] + be_i gl[t_i]) with al/be the
// integrals of the nodal coefficients (Interpolant::integrate, Functions.hh:246-253).
// K10: per-element averaged strain / stress (LinearElasticity.hh:99-123, :528-549).
// ------------------------------------------------------------------------------------------------
template <int DIM>
DEV void load_corner_perturbation(const double *__restrict__ g, const int32_t *__restrict__ en, const double *__restrict__ deltaP,
                                  double (&gl)[DIM + 1][DIM], double (&dgl)[DIM + 1][DIM], double &relDeltaVol);

struct LoadArgs {
    int64_t nElem;
    int npe, geoStride;
    const double *geo;
    const int32_t *elemNodes;
    const int32_t *dofForNode;   // may be null
    double intGrad[20];          // npe x {al, be}
    double cstrain[6];           // flattened, TENSOR shear
};

template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_constant_strain_load(LoadArgs a, const double *__restrict__ deltaP, double *__restrict__ out) {
    constexpr int FL = DIM * (DIM + 1) / 2;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    const int64_t total = a.nElem * NPE;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
        const int64_t e = k / NPE;
        const int i = (int)(k - e * NPE);
        const double *g = a.geo + e * a.geoStride;
        double sd[FL], cs[FL];
#pragma unroll
        for (int q = 0; q < FL; ++q) sd[q] = a.cstrain[q] * (q < DIM ? 1.0 : 2.0);   // shearDoubled (ElasticityTensor.hh:437-441)
        elem_D_apply<DIM, MAT>(g, sd, cs);
        const int si = sup_s<DIM, DEG>(i), ti = sup_t<DIM, DEG>(i);
        const double vol = g[12];
        // runtime-indexed kernel-argument array: read through a select chain over the small table
        double al = 0, be = 0;
#pragma unroll
        for (int q = 0; q < NPE; ++q) { al = (q == i) ? a.intGrad[2 * q] : al; be = (q == i) ? a.intGrad[2 * q + 1] : be; }
        double gi[DIM];
        if (deltaP) {
            // deltaConstantStrainLoad (LinearElasticity.hh:289-304, :1331-1348): delta (vol grad lambda) = vol (rel gl + dgl)
            double gl[DIM + 1][DIM], dgl[DIM + 1][DIM], rel;
            load_corner_perturbation<DIM>(g, a.elemNodes + e * NPE, deltaP, gl, dgl, rel);
            double gs[DIM], gt[DIM];
#pragma unroll
            for (int b = 0; b < DIM; ++b) { gs[b] = 0.0; gt[b] = 0.0; }
#pragma unroll
            for (int k2 = 0; k2 < DIM + 1; ++k2)
#pragma unroll
                for (int b = 0; b < DIM; ++b) {
                    const double v = rel * gl[k2][b] + dgl[k2][b];
                    gs[b] = (k2 == si) ? v : gs[b];
                    gt[b] = (k2 == ti) ? v : gt[b];
                }
#pragma unroll
            for (int b = 0; b < DIM; ++b) gi[b] = vol * (al * gs[b] + be * gt[b]);
        } else {
#pragma unroll
            for (int b = 0; b < DIM; ++b) gi[b] = vol * (al * g[si * DIM + b] + be * g[ti * DIM + b]);
        }
        int64_t dof = a.elemNodes[e * NPE + i];
        if (a.dofForNode) dof = a.dofForNode[dof];
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            double v = 0;
#pragma unroll
            for (int b = 0; b < DIM; ++b) v += cs[flat_idx<DIM>(c, b)] * gi[b];
            unsafeAtomicAdd(&out[dof * DIM + c], v);
        }
    }
}

// Stretch of a mesh as a whole (MFH_PRECOND_AUTO): M = sum over the elements of sum over their edges of e e^T (flattened xx, yy, zz, yz, xz, xy). An
// isotropic mesh -- whatever the shapes of its elements, as long as their directions average out -- has M ~ I; a mesh stretched s : 1 : 1 has
// eigenvalues ~ (s^2, 1, 1). One lane per element, sums through the wave and one atomic per wave and entry.
__global__ void __launch_bounds__(256) k_edge_covariance(int64_t nElem, int dim, int npe, const int32_t *__restrict__ elemNodes, const double *__restrict__ vertPos,
                                                        double *__restrict__ out6) {
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nElem; e += (int64_t)gridDim.x * 256) {
        double P[4][3];
        for (int k = 0; k <= dim; ++k) {
            const int64_t v = elemNodes[e * npe + k];
            for (int a = 0; a < 3; ++a) P[k][a] = a < dim ? vertPos[v * dim + a] : 0.0;
        }
        for (int i = 0; i <= dim; ++i)
            for (int j = i + 1; j <= dim; ++j) {
                const double x = P[j][0] - P[i][0], y = P[j][1] - P[i][1], z = P[j][2] - P[i][2];
                acc[0] += x * x; acc[1] += y * y; acc[2] += z * z; acc[3] += y * z; acc[4] += x * z; acc[5] += x * y;
            }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double v = wave_sum(acc[q]);
        if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(&out6[q], v);
    }
}

// K8, neumannLoad (LinearElasticity.hh:703-717): f[DoF(node)] += traction_b * int phi_n over boundary element b, one lane per (boundary element,
// local node); int phi_n = w[n] * |b| with the weights of Functions.hh:246-274 (kernel argument). The boundary of a mesh is a few per cent of
// its nodes: global atomics are fine here. The vector stays on the device: it is the right-hand side of the solve that follows.
struct NeumannArgs { int64_t nBE; int npbe, dim; double w[6]; };
__global__ void __launch_bounds__(256) k_neumann_load(NeumannArgs a, const int32_t *__restrict__ bdryElemNodes, const int32_t *__restrict__ dofForNode,
                                                      const double *__restrict__ bdryVol, const double *__restrict__ traction, double *__restrict__ out) {
    const int64_t total = a.nBE * a.npbe;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t b = q / a.npbe;
        const int k = (int)(q - b * a.npbe);
        double wk = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) wk = (j == k) ? a.w[j] : wk;
        if (wk == 0.0) continue;
        int64_t dof = bdryElemNodes[q];
        if (dofForNode) dof = dofForNode[dof];
        const double wv = wk * bdryVol[b];
        for (int c = 0; c < a.dim; ++c) {
            const double t = traction[b * a.dim + c];
            if (t != 0.0) unsafeAtomicAdd(&out[dof * a.dim + c], wv * t);
        }
    }
}

// add.on: a constant strain (flattened, TENSOR shear) is added to every element's average strain -- the strain of the affine field
// x -> E x, which then never has to exist as a nodal vector. integral != null: sum_e vol_e * (the element's result) is accumulated
// there (FL doubles, zeroed by the caller) and `out` may be null: the per-element field stays in registers.
struct StrainShift { double v[6]; int on; };
template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_average_strain(LoadArgs a, const double *__restrict__ uNodes, double *__restrict__ out,
                                                        int wantStress, const double *__restrict__ uFixed,
                                                        const double *__restrict__ deltaP, StrainShift add, double *__restrict__ integral) {
    constexpr int FL = DIM * (DIM + 1) / 2;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    __shared__ double red[12];
    double total[FL];
#pragma unroll
    for (int q = 0; q < FL; ++q) total[q] = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.nElem; e += (int64_t)gridDim.x * 256) {
        const double *g = a.geo + e * a.geoStride;
        double eps[DIM][DIM];
#pragma unroll
        for (int x = 0; x < DIM; ++x)
#pragma unroll
            for (int y = 0; y < DIM; ++y) eps[x][y] = 0.0;
#pragma unroll
        for (int i = 0; i < NPE; ++i) {
            const int si = sup_s<DIM, DEG>(i), ti = sup_t<DIM, DEG>(i);
            const double al = a.intGrad[2 * i], be = a.intGrad[2 * i + 1];
            const int64_t node = a.elemNodes[e * NPE + i];
            double gb[DIM], ui[DIM];
#pragma unroll
            for (int b = 0; b < DIM; ++b) { gb[b] = al * g[si * DIM + b] + be * g[ti * DIM + b]; ui[b] = uNodes[node * DIM + b]; }
#pragma unroll
            for (int x = 0; x < DIM; ++x)
#pragma unroll
                for (int y = 0; y < DIM; ++y) eps[x][y] += 0.5 * (ui[x] * gb[y] + ui[y] * gb[x]);   // LinearElasticity.hh:99-115
        }
        if (deltaP) {
            // deltaAverageStrainField (LinearElasticity.hh:1364-1374): + (delta strain)(uFixed), the strain of the fixed
            // field on the perturbed gradients (:259-277)
            double gl[DIM + 1][DIM], dgl[DIM + 1][DIM], rel;
            load_corner_perturbation<DIM>(g, a.elemNodes + e * NPE, deltaP, gl, dgl, rel);
#pragma unroll
            for (int i = 0; i < NPE; ++i) {
                const int si = sup_s<DIM, DEG>(i), ti = sup_t<DIM, DEG>(i);
                const double al = a.intGrad[2 * i], be = a.intGrad[2 * i + 1];
                const int64_t node = a.elemNodes[e * NPE + i];
                double gb[DIM], ui[DIM];
#pragma unroll
                for (int b = 0; b < DIM; ++b) { gb[b] = al * dgl[si][b] + be * dgl[ti][b]; ui[b] = uFixed[node * DIM + b]; }
#pragma unroll
                for (int x = 0; x < DIM; ++x)
#pragma unroll
                    for (int y = 0; y < DIM; ++y) eps[x][y] += 0.5 * (ui[x] * gb[y] + ui[y] * gb[x]);
            }
        }
        double ef[FL];
#pragma unroll
        for (int x = 0; x < DIM; ++x)
#pragma unroll
            for (int y = x; y < DIM; ++y) ef[flat_idx<DIM>(x, y)] = eps[x][y];
        if (add.on)
#pragma unroll
            for (int q = 0; q < FL; ++q) ef[q] += add.v[q];
        if (wantStress) {
            double sd[FL], sg[FL];
#pragma unroll
            for (int q = 0; q < FL; ++q) sd[q] = ef[q] * (q < DIM ? 1.0 : 2.0);
            elem_D_apply<DIM, MAT>(g, sd, sg);
#pragma unroll
            for (int q = 0; q < FL; ++q) ef[q] = sg[q];
        }
        if (out)
#pragma unroll
            for (int q = 0; q < FL; ++q) out[e * FL + q] = ef[q];
        if (integral) {
            const double vol = g[12];
#pragma unroll
            for (int q = 0; q < FL; ++q) total[q] += vol * ef[q];
        }
    }
    if (integral) {
#pragma unroll
        for (int h = 0; h < FL; h += 3) {
            double v[3] = {total[h], total[h + 1], total[h + 2]};
            block_sum<3>(v, red);
            if (threadIdx.x == 0)
#pragma unroll
                for (int q = 0; q < 3; ++q) unsafeAtomicAdd(&integral[h + q], v[q]);
        }
    }
}

// Average gradient of a scalar nodal field per element (PoissonMesh::gradUAverage, Poisson.hh:121-131):
// (1/vol) int sum_i u_i grad phi_i = sum_i u_i (al_i gl[s_i] + be_i gl[t_i]).
template <int DIM, int DEG>
__global__ void __launch_bounds__(256) k_average_gradient(LoadArgs a, const double *__restrict__ uNodes, double *__restrict__ out) {
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.nElem; e += (int64_t)gridDim.x * 256) {
        const double *g = a.geo + e * a.geoStride;
        double gr[DIM];
#pragma unroll
        for (int b = 0; b < DIM; ++b) gr[b] = 0.0;
#pragma unroll
        for (int i = 0; i < NPE; ++i) {
            const int si = sup_s<DIM, DEG>(i), ti = sup_t<DIM, DEG>(i);
            const double al = a.intGrad[2 * i], be = a.intGrad[2 * i + 1];
            const double ui = uNodes[a.elemNodes[e * NPE + i]];
#pragma unroll
            for (int b = 0; b < DIM; ++b) gr[b] += ui * (al * g[si * DIM + b] + be * g[ti * DIM + b]);
        }
#pragma unroll
        for (int b = 0; b < DIM; ++b) out[e * DIM + b] = gr[b];
    }
}

// ------------------------------------------------------------------------------------------------
// Block-CSR SpMV over row chunks (persistent workgroups, grid-stride over chunks).
// Phase 1: lane per block: coalesced loads of the NB components + column, gather x, block product
//          -> LDS partials.  Phase 2: lane per scalar row sums its partials.
// Optional: zero rows of fixed variables; accumulate dot(x_rows, y) into *dotOut (one atomic per WG).
// ------------------------------------------------------------------------------------------------
template <int DIM, int PCG>
__global__ void __launch_bounds__(256) k_spmv(SpmvArgs a, const double *__restrict__ x, double *__restrict__ y,
                                             double *dotOut, double *scal, int it, const double *stopPtr, const int32_t *__restrict__ chunkList,
                                             int64_t nList) {
    constexpr int NB = DIM * DIM;
    extern __shared__ __attribute__((aligned(16))) double part[];  // [DIM][chunkSlots] + 16
    const int CS = a.chunkSlots;
    double *red = part + DIM * CS;
    if (PCG == 1) {
        it += (int)stopPtr[3];   // iteration base of the current graph launch (0 outside graphs)
        // converged: every kernel of the remaining iterations is a no-op
        if (scal[(int64_t)it * 4 + 2] <= stopPtr[0]) return;
        dotOut = scal + (int64_t)it * 4 + 1;
    } else if (PCG == 2) {   // Chronopoulos-Gear bookkeeping for one right-hand side (see k_spmv_nr)
        it += (int)stopPtr[0];
        if (scal[(int64_t)it * 4 + 2] <= stopPtr[2]) return;
        dotOut = scal + (int64_t)(it + 1) * 4 + 1;
    }
    double dot = 0.0;
    int64_t chunkFirst = blockIdx.x, chunkEnd = chunkList ? nList : a.nChunk, chunkStride = gridDim.x;
    if (a.xcd && !chunkList) xcd_span(a.nChunk, chunkFirst, chunkEnd, chunkStride);
    for (int64_t cq = chunkFirst; cq < chunkEnd; cq += chunkStride) {
        const int64_t chunk = chunkList ? (int64_t)chunkList[cq] : cq;
        const int r0 = a.chunkRow[chunk], r1 = a.chunkRow[chunk + 1];
        const int s0 = a.rowPtr[r0];
        const int ns = a.rowPtr[r1] - s0;
        for (int t = threadIdx.x; t < ns; t += 256) {
            const int64_t s = (int64_t)s0 + t;
            const int64_t col = a.colIdx[s];
            double xv[DIM], A[NB];
            if (a.vals32) {              // (uniform over the launch: the FP32 copy of the matrix, SpmvArgs)
#pragma unroll
                for (int c = 0; c < NB; ++c) A[c] = (double)a.vals32[tiled_index(s, c, NB)];
            } else {
#pragma unroll
                for (int c = 0; c < NB; ++c) A[c] = a.vals[tiled_index(s, c, NB)];
            }
#pragma unroll
            for (int d = 0; d < DIM; ++d) xv[d] = x[col * DIM + d];
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                double v = 0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) v += A[c * DIM + d] * xv[d];
                part[c * CS + t] = v;
            }
        }
        __syncthreads();
        const int nscalar = (r1 - r0) * DIM;
        for (int idx = threadIdx.x; idx < nscalar; idx += 256) {
            const int rl = idx / DIM, c = idx - rl * DIM;
            const int64_t r = r0 + rl;
            const int b = a.rowPtr[r] - s0, e = a.rowPtr[r + 1] - s0;
            double v = 0;
            for (int t = b; t < e; ++t) v += part[c * CS + t];
            const int64_t gi = r * DIM + c;
            if (a.fixedMask && a.fixedMask[gi]) v = 0.0;
            y[gi] = v;
            if (dotOut) dot += v * x[gi];
        }
        __syncthreads();
    }
    if (dotOut) {
        double v[1] = {dot};
        block_sum<1>(v, red);
        double *const tg[1] = {dotOut};
        commit_sums<1>(v, tg, a.det, red);
    }
}

// ------------------------------------------------------------------------------------------------
// y = (M (x) I_N) x for a matrix stored as ONE value per block (MFH_OP_MASS_VECTOR; MassMatrix::construct_vector_valued,
// MassMatrix.hh:131-147): y[N i + c] = sum_j m_ij x[N j + c]. The row chunks, the LDS partials, the fixed-variable mask and the fused dot
// product / PCG bookkeeping are k_spmv's; a stored block costs 8 bytes of matrix + 4 of column index instead of 8 N^2 + 4. The lanes of a
// wave take consecutive stored blocks of the chunk (the values and columns are read as contiguous runs); the N components of an x row are
// adjacent 8-byte reads of one lane (array-of-rows vectors, as everywhere in the solver). No atomics: two applications give the same bits.
// Not taken over from k_spmv: the XCD-contiguous chunk mapping (a.xcd is ignored: measured slower there) and the FP32 copy of the values
// (a.vals32: a multigrid-smoother device, and this operator has no hierarchy); PCG is 0 (plain) or 1 (classic loop) -- the launcher
// refuses the Chronopoulos-Gear bookkeeping.
// ------------------------------------------------------------------------------------------------
template <int N, int PCG>
__global__ void __launch_bounds__(256) k_spmv_kron(SpmvArgs a, const double *__restrict__ x, double *__restrict__ y,
                                                  double *dotOut, double *scal, int it, const double *stopPtr, const int32_t *__restrict__ chunkList,
                                                  int64_t nList) {
    extern __shared__ __attribute__((aligned(16))) double part[];  // [N][chunkSlots] + 16
    const int CS = a.chunkSlots;
    double *red = part + N * CS;
    if (PCG == 1) {
        it += (int)stopPtr[3];
        if (scal[(int64_t)it * 4 + 2] <= stopPtr[0]) return;
        dotOut = scal + (int64_t)it * 4 + 1;
    }
    double dot = 0.0;
    const int64_t chunkEnd = chunkList ? nList : a.nChunk;
    for (int64_t cq = blockIdx.x; cq < chunkEnd; cq += gridDim.x) {
        const int64_t chunk = chunkList ? (int64_t)chunkList[cq] : cq;
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
            if (a.fixedMask && a.fixedMask[gi]) v = 0.0;
            y[gi] = v;
            if (dotOut) dot += v * x[gi];
        }
        __syncthreads();
    }
    if (dotOut) {
        double v[1] = {dot};
        block_sum<1>(v, red);
        double *const tg[1] = {dotOut};
        commit_sums<1>(v, tg, a.det, red);
    }
}

// Row sums of a matrix with one value per block: the lumped mass matrix (MassMatrix.hh:104-127), repeated `rep` times per row for the
// vector-valued operator. UPPER: only the entries (r, c >= r) are stored and an off-diagonal one belongs to both rows (MassMatrix.hh:113-117);
// the mirrored half goes to the other row with a global atomic (out zeroed by the caller), like k_spmv_sym's transposed products -- in
// arrival order, so mfh_mass_lumped refuses that path under option "deterministic". One lane per row walks its values and columns
// uncoalesced: a one-off call per mesh, not an operator of the PCG.
template <bool UPPER>
__global__ void __launch_bounds__(256) k_row_sums(int64_t nRows, const int32_t *__restrict__ rowPtr, const int32_t *__restrict__ colIdx,
                                                 const double *__restrict__ vals, int rep, double *__restrict__ out) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nRows; r += (int64_t)gridDim.x * 256) {
        double v = 0;
        for (int q = rowPtr[r]; q < rowPtr[r + 1]; ++q) {
            const double m = vals[tiled_index(q, 0, 1)];
            v += m;
            if (UPPER) {
                const int64_t col = colIdx[q];
                if (col != r && col < nRows)
                    for (int c = 0; c < rep; ++c) unsafeAtomicAdd(&out[col * rep + c], m);
            }
        }
        for (int c = 0; c < rep; ++c) {
            if (UPPER) unsafeAtomicAdd(&out[r * rep + c], v);
            else out[r * rep + c] = v;
        }
    }
}

// Discrete divergence of a per-element vector field on linear elements (the reference's python binding differential_operators.cc:79-88):
// out[n] = sum_{e containing n} v_e . int_e grad phi_n = sum vol_e v_e . grad lambda_i. Gather form: one lane per node walks the node's
// (element, local node) pairs; nothing is added atomically.
template <int DIM>
__global__ void __launch_bounds__(256) k_divergence(int64_t nNode, const int32_t *__restrict__ nodePtr, const int32_t *__restrict__ nodePair,
                                                   const double *__restrict__ geo, int geoStride, const double *__restrict__ elemVec,
                                                   double *__restrict__ out) {
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < nNode; n += (int64_t)gridDim.x * 256) {
        double v = 0;
        for (int q = nodePtr[n]; q < nodePtr[n + 1]; ++q) {
            const int64_t code = nodePair[q], e = code / (DIM + 1);
            const int i = (int)(code - e * (DIM + 1));
            const double *g = geo + e * geoStride;
            double w = 0;
#pragma unroll
            for (int b = 0; b < DIM; ++b) w += elemVec[e * DIM + b] * g[i * DIM + b];
            v += g[12] * w;
        }
        out[n] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// y = K x from the UPPER-TRIANGLE storage (blocks (r, c >= r): what the reference's TripletMatrix holds, SparseMatrices.hh:231-234) -- the
// "symmetric-storage SpMV" of VERDICT r3 item 7. Same chunks as k_spmv. A stored off-diagonal block serves twice: A x_c goes to the row's
// LDS partial as in k_spmv, A^T x_r is ADDED to y_c -- a row of another chunk (in the lattice order of the generator's meshes the columns of a
// row lie up to a plane of the grid away), hence a global FP64 atomic; the rows' own sums are added atomically too (other workgroups scatter into
// them), y is zeroed by the launcher. Half the matrix bytes of k_spmv, plus 3 atomics per off-diagonal block.
// ------------------------------------------------------------------------------------------------
template <int DIM>
__global__ void __launch_bounds__(256) k_spmv_sym(SpmvArgs a, int64_t nRows, const double *__restrict__ x, double *__restrict__ y) {
    constexpr int NB = DIM * DIM;
    extern __shared__ __attribute__((aligned(16))) double part[];  // [DIM][chunkSlots] + row of every slot (u16)
    const int CS = a.chunkSlots;
    unsigned short *rowOf = reinterpret_cast<unsigned short *>(part + DIM * CS);
    int64_t chunkFirst = blockIdx.x, chunkEnd = a.nChunk, chunkStride = gridDim.x;
    if (a.xcd) xcd_span(a.nChunk, chunkFirst, chunkEnd, chunkStride);
    for (int64_t chunk = chunkFirst; chunk < chunkEnd; chunk += chunkStride) {
        const int r0 = a.chunkRow[chunk], r1 = a.chunkRow[chunk + 1];
        const int s0 = a.rowPtr[r0];
        const int ns = a.rowPtr[r1] - s0;
        for (int rl = threadIdx.x; rl < r1 - r0; rl += 256) {
            const int b = a.rowPtr[r0 + rl] - s0, e = a.rowPtr[r0 + rl + 1] - s0;
            for (int t = b; t < e; ++t) rowOf[t] = (unsigned short)rl;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < ns; t += 256) {
            const int64_t s = (int64_t)s0 + t;
            const int64_t col = a.colIdx[s], row = r0 + rowOf[t];
            double xc[DIM], xr[DIM], A[NB];
#pragma unroll
            for (int c = 0; c < NB; ++c) A[c] = a.vals[tiled_index(s, c, NB)];
#pragma unroll
            for (int d = 0; d < DIM; ++d) { xc[d] = x[col * DIM + d]; xr[d] = x[row * DIM + d]; }
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                double v = 0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) v += A[c * DIM + d] * xc[d];
                part[c * CS + t] = v;
            }
            if (col != row && col < nRows) {     // (a halo column's row belongs to another rank, which stores the block itself)
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    double w = 0;
#pragma unroll
                    for (int c = 0; c < DIM; ++c) w += A[c * DIM + d] * xr[c];
                    const int64_t gj = col * DIM + d;
                    if (!(a.fixedMask && a.fixedMask[gj])) unsafeAtomicAdd(&y[gj], w);
                }
            }
        }
        __syncthreads();
        const int nscalar = (r1 - r0) * DIM;
        for (int idx = threadIdx.x; idx < nscalar; idx += 256) {
            const int rl = idx / DIM, c = idx - rl * DIM;
            const int64_t r = r0 + rl;
            const int b = a.rowPtr[r] - s0, e = a.rowPtr[r + 1] - s0;
            double v = 0;
            for (int t = b; t < e; ++t) v += part[c * CS + t];
            const int64_t gi = r * DIM + c;
            if (!(a.fixedMask && a.fixedMask[gi])) unsafeAtomicAdd(&y[gi], v);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// Matrix-free operator y = K x: one lane per (element, local node i) pair evaluates the row i of the
// element matrix block by block in registers (same elem_block as the assembly: identical values) and
// applies it to the gathered x; pairs of a row chunk are reduced in LDS. Trades the 72 B/block of the
// assembled SpMV for ~73 FP64 flops/block: HBM traffic drops from nnzb*76 B to the element records +
// pair lists + x, the FP64 VALU (idle in the assembled SpMV) does the work.
// ------------------------------------------------------------------------------------------------
template <int DIM, int DEG, int MAT, bool PCG>
__global__ void __launch_bounds__(256) k_spmv_mf(SpmvMfArgs a, const double *__restrict__ x, double *__restrict__ y, double *dotOut,
                                                 double *scal, int it, const double *stopPtr) {
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr int NB = mat_nb<DIM, MAT>();
    constexpr int BS = NB == 1 ? 1 : DIM;
    extern __shared__ __attribute__((aligned(16))) double mfacc[];   // [maxRows * BS] + 16
    double *red = mfacc + a.maxRows * BS;
    if (PCG) {
        it += (int)stopPtr[3];
        if (scal[(int64_t)it * 4 + 2] <= stopPtr[0]) return;
        dotOut = scal + (int64_t)it * 4 + 1;
    }
    const PairConst pc{a.pairConst[0], a.pairConst[1], a.pairConst[2], a.pairConst[3], a.pairConst[4], a.pairConst[5]};
    const double *tab = MAT == MAT_MASS ? a.massTable : a.pairTable;
    double dot = 0.0;
    int64_t chunkFirst = blockIdx.x, chunkEnd = a.nChunk, chunkStride = gridDim.x;
    if (a.xcd) xcd_span(a.nChunk, chunkFirst, chunkEnd, chunkStride);
    for (int64_t chunk = chunkFirst; chunk < chunkEnd; chunk += chunkStride) {
        const int r0 = a.chunkRow[chunk], r1 = a.chunkRow[chunk + 1];
        const int nr = (r1 - r0) * BS;
        for (int t = threadIdx.x; t < nr; t += 256) mfacc[t] = 0.0;
        __syncthreads();
        const int64_t kb = a.pairPtr[chunk], ke = a.pairPtr[chunk + 1];
        for (int64_t k = kb + threadIdx.x; k < ke; k += 256) {
            const uint32_t code = a.pairCode[k];
            const int lr = a.pairRow[k];
            const uint32_t e = code / NPE;
            const int i = (int)(code - e * NPE);
            const double *g = a.geo + (int64_t)e * a.geoStride;
            const int32_t *en = a.elemNodes + (int64_t)e * NPE;
            double out[BS];
#pragma unroll
            for (int c = 0; c < BS; ++c) out[c] = 0.0;
#pragma unroll
            for (int j = 0; j < NPE; ++j) {
                int64_t col = en[j];
                if (a.dofForNode) col = a.dofForNode[col];
                double xv[BS], K[NB];
#pragma unroll
                for (int d = 0; d < BS; ++d) xv[d] = x[col * BS + d];
                elem_block<DIM, DEG, MAT>(g, tab, pc, i, j, K);
#pragma unroll
                for (int c = 0; c < BS; ++c)
#pragma unroll
                    for (int d = 0; d < BS; ++d) out[c] += K[c * BS + d] * xv[d];
            }
#pragma unroll
            for (int c = 0; c < BS; ++c) unsafeAtomicAdd(&mfacc[lr * BS + c], out[c]);
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < nr; idx += 256) {
            const int64_t gi = (int64_t)r0 * BS + idx;
            double v = mfacc[idx];
            if (a.fixedMask && a.fixedMask[gi]) v = 0.0;
            y[gi] = v;
            if (dotOut) dot += v * x[gi];
        }
        __syncthreads();
    }
    if (dotOut) {
        double v[1] = {dot};
        block_sum<1>(v, red);
        double *const tg[1] = {dotOut};
        commit_sums<1>(v, tg, a.det, red);
    }
}

// ------------------------------------------------------------------------------------------------
// Matrix-free ELASTICITY operator in two passes -- the stresses are shared by the npe rows of an element
// instead of being recomputed per (element, node) pair:
//   k_mf_forces: one lane per element. With the reference's quadrature rule every point q belongs to a vertex
//     (lambda_k(q) = c0 if k == q else c1), so grad u(q) = G_b + (a-b) x_q (x) gl_q + (A-B) sum_{k != q} x_edge(k,q) (x) gl_k
//     with G_b = sum_k (b x_k + B sum_{edges m at k} x_m) (x) gl_k,  a = 4 c0 - 1, b = 4 c1 - 1, A = 4 c0, B = 4 c1
//     (EmbeddedElement.hh:288-313). With S' = vol w sum_q sigma_q and R_q = vol w (a-b) sigma_q the nodal forces
//     f_i = int sigma(u) grad phi_i are
//     vertex k: (b S' + R_k) gl_k ;  edge (s,t): (B S' + R_t) gl_s + (B S' + R_s) gl_t ;  P1: vol sigma gl_i
//     (same quadrature as the assembled K: identical up to rounding), written element-major: 240 B per P2 tet.
//   k_mf_rows: one lane per (element, node) pair (lists of build_mf_lists_device): y_row = sum of the pairs' forces
//     -- a pure gather-sum through LDS, no arithmetic.
// HBM traffic: records + connectivity + x + 2 x 240 B/element of forces + pair lists ~ 4.5 GB at 5.2 M P2 tets,
// against 15.7 GB for the assembled SpMV.
// ------------------------------------------------------------------------------------------------
template <int DIM> DEV constexpr int edge_between(int k, int q) {
    // local edge index joining vertices k and q (Simplex.hh:43-47): (0,1),(1,2),(2,0),(0,3),(2,3),(1,3)
    const int lo = k < q ? k : q, hi = k < q ? q : k;
    if (lo == 0 && hi == 1) return 0;
    if (lo == 1 && hi == 2) return 1;
    if (lo == 0 && hi == 2) return 2;
    if (lo == 0 && hi == 3) return 3;
    if (lo == 2 && hi == 3) return 4;
    return 5;   // (1,3)
}

// nodal forces f_i = int sigma(u) grad phi_i of element e for the nodal vectors gathered from x
template <int DIM, int DEG, int MAT, bool SHIFT = false, class Emit>
DEV void elem_forces_core(const SpmvMfArgs &a, int64_t e, const double (&xl)[(DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6)][DIM],
                          const Emit &emit);

template <int DIM, int DEG, int MAT>
DEV void elem_forces(const SpmvMfArgs &a, int64_t e, const double *__restrict__ x,
                     double (&f)[(DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6)][DIM]) {
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    const int32_t *en = a.elemNodes + e * NPE;
    double xl[NPE][DIM];
#pragma unroll
    for (int j = 0; j < NPE; ++j) {
        int64_t col = en[j];
        if (a.dofForNode) col = a.dofForNode[col];
#pragma unroll
        for (int d = 0; d < DIM; ++d) xl[j][d] = x[col * DIM + d];
    }
    elem_forces_core<DIM, DEG, MAT>(a, e, xl, [&](int j, const double *fv) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) f[j][d] = fv[d];
    });
}

// The arithmetic of elem_forces on nodal vectors that are already gathered, as a bilinear form in the barycentric
// gradients: the strain of u is built with glS, the test functions' gradients with glT,
//     f_i = vol int sigma(u; glS) grad phi_i(glT).
// The operator itself is glS == glT == grad lambda; the discrete shape derivative (k_apply_delta_K) feeds perturbed
// gradients into either slot. Every nodal force is handed to `emit(j, f_j)` as soon as it is complete (the cluster
// kernel adds it to LDS right away instead of keeping 30 values live).
// SHIFT: the constant strain `shift` (flattened, tensor shear; a kernel argument) is added to grad u at every point -- with u = 0 the nodal
// forces are constantStrainLoad's (LinearElasticity.hh:551-562).
template <int DIM, int DEG, int MAT, bool SHIFT = false, class Emit>
DEV void elem_forces_bilinear(const double *__restrict__ g /* element record: material */, double vol,
                              const double (&gl)[DIM + 1][DIM], const double (&glT)[DIM + 1][DIM],
                              const double (&xl)[(DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6)][DIM], const Emit &emit,
                              const double *shift = nullptr) {
    constexpr int NV = DIM + 1;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr int FL = DIM * (DIM + 1) / 2;
    auto stress_of = [&](const double (&G)[DIM][DIM], double *out) {
        double sd[FL];
#pragma unroll
        for (int p = 0; p < DIM; ++p)
#pragma unroll
            for (int q2 = p; q2 < DIM; ++q2)
                sd[flat_idx<DIM>(p, q2)] = (p == q2) ? G[p][p] : (G[p][q2] + G[q2][p]);   // shear-doubled strain
        elem_D_apply<DIM, MAT>(g, sd, out);
    };
    auto symv = [&](const double *T, const double *v, double *o) {   // o += T v  (T flat symmetric)
#pragma unroll
        for (int p = 0; p < DIM; ++p)
#pragma unroll
            for (int q2 = 0; q2 < DIM; ++q2) o[p] += T[flat_idx<DIM>(p, q2)] * v[q2];
    };
    if (DEG == 1) {
        double G[DIM][DIM];
#pragma unroll
        for (int p = 0; p < DIM; ++p)
#pragma unroll
            for (int q2 = 0; q2 < DIM; ++q2) {
                double v = 0;
#pragma unroll
                for (int j = 0; j < NV; ++j) v += xl[j][p] * gl[j][q2];
                if (SHIFT) v += shift[flat_idx<DIM>(p, q2)];
                G[p][q2] = v;
            }
        double sg[FL];
        stress_of(G, sg);
#pragma unroll
        for (int c = 0; c < FL; ++c) sg[c] *= vol;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            double fv[DIM] = {};
            symv(sg, glT[j], fv);
            emit(j, fv);
        }
    } else {
        constexpr double c0 = DIM == 3 ? 0.58541019662496845446 : 2.0 / 3.0;     // GaussQuadrature.hh:283-295 / :115-127
        constexpr double c1 = DIM == 3 ? 0.13819660112501051518 : 1.0 / 6.0;
        constexpr double b_ = 4 * c1 - 1, A_ = 4 * c0, B_ = 4 * c1, dAB = A_ - B_;   // a - b = A - B
        constexpr double wq = 1.0 / NV;
        double Gb[DIM][DIM];
#pragma unroll
        for (int p = 0; p < DIM; ++p)
#pragma unroll
            for (int q2 = 0; q2 < DIM; ++q2) Gb[p][q2] = SHIFT ? shift[flat_idx<DIM>(p, q2)] : 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double base[DIM];
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                double sum = 0;
#pragma unroll
                for (int o = 0; o < NV; ++o)
                    if (o != k) sum += xl[NV + edge_between<DIM>(k, o)][d];
                base[d] = b_ * xl[k][d] + B_ * sum;
            }
#pragma unroll
            for (int p = 0; p < DIM; ++p)
#pragma unroll
                for (int q2 = 0; q2 < DIM; ++q2) Gb[p][q2] += base[p] * gl[k][q2];
        }
        double S[FL], R[NV][FL];
#pragma unroll
        for (int c = 0; c < FL; ++c) S[c] = 0.0;
        // Material flavours with more than two parameters (orthotropic: 9 doubles, general: 21): the four point strains are formed FIRST,
        // with no material value live, and the tensor is fetched only once the 30 gathered nodal values are dead -- otherwise the
        // scheduler requests the record's material part up front and the kernel needs 186 / 210 VGPRs (2 waves per SIMD) instead of the
        // isotropic flavour's 166 (3 waves). The opaque asm ties the record pointer to the last strain, so no load can move above it.
        if (MAT != MAT_ISO) {
#pragma unroll
            for (int q = 0; q < NV; ++q) {
#pragma unroll
                for (int p = 0; p < DIM; ++p)
#pragma unroll
                    for (int q2 = p; q2 < DIM; ++q2) {
                        double v = 0;
#pragma unroll
                        for (int side = 0; side < (p == q2 ? 1 : 2); ++side) {
                            const int r = side ? q2 : p, cc = side ? p : q2;
                            double w = Gb[r][cc] + dAB * xl[q][r] * gl[q][cc];
#pragma unroll
                            for (int k = 0; k < NV; ++k)
                                if (k != q) w += dAB * xl[NV + edge_between<DIM>(k, q)][r] * gl[k][cc];
                            v += w;
                        }
                        R[q][flat_idx<DIM>(p, q2)] = v;                     // shear-doubled flat strain of point q
                    }
            }
            const double *gm = g;
            asm volatile("" : "+v"(gm), "+v"(R[NV - 1][FL - 1]), "+v"(R[0][0]));
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                double sg[FL];
                elem_D_apply<DIM, MAT>(gm, R[q], sg);
#pragma unroll
                for (int c = 0; c < FL; ++c) { S[c] += sg[c]; R[q][c] = vol * wq * dAB * sg[c]; }
                // (general tensors: a scheduling barrier here -- one point after the other -- brings the kernel from 204 to 160 VGPRs, 3 waves per SIMD, and
                // from 0.32 to 0.48 ms at 2 M tets: the 21 tensor loads of a point then wait for each other instead of running ahead. Measured, not adopted.)
            }
        } else
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            double G[DIM][DIM];
#pragma unroll
            for (int p = 0; p < DIM; ++p)
#pragma unroll
                for (int q2 = 0; q2 < DIM; ++q2) {
                    double v = Gb[p][q2] + dAB * xl[q][p] * gl[q][q2];
#pragma unroll
                    for (int k = 0; k < NV; ++k)
                        if (k != q) v += dAB * xl[NV + edge_between<DIM>(k, q)][p] * gl[k][q2];
                    G[p][q2] = v;
                }
            double sg[FL];
            stress_of(G, sg);
#pragma unroll
            for (int c = 0; c < FL; ++c) { S[c] += sg[c]; R[q][c] = vol * wq * dAB * sg[c]; }
        }
        // vertex k: f = (b S' + R_k) gl_k ;  edge (s,t): f = (B S' + R_t) gl_s + (B S' + R_s) gl_t
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double T[FL];
#pragma unroll
            for (int c = 0; c < FL; ++c) T[c] = (vol * wq * b_) * S[c] + R[k][c];
            double fv[DIM] = {};
            symv(T, glT[k], fv);
            emit(k, fv);
        }
#pragma unroll
        for (int c = 0; c < FL; ++c) S[c] *= vol * wq * B_;
#pragma unroll
        for (int m = 0; m < NPE - NV; ++m) {
            const int sI = sup_s<DIM, DEG>(NV + m), tI = sup_t<DIM, DEG>(NV + m);
            double T1[FL], T2[FL];
#pragma unroll
            for (int c = 0; c < FL; ++c) { T1[c] = S[c] + R[tI][c]; T2[c] = S[c] + R[sI][c]; }
            double fv[DIM] = {};
            symv(T1, glT[sI], fv);
            symv(T2, glT[tI], fv);
            emit(NV + m, fv);
        }
    }
}

template <int DIM, int DEG, int MAT, bool SHIFT, class Emit>
DEV void elem_forces_core(const SpmvMfArgs &a, int64_t e, const double (&xl)[(DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6)][DIM],
                          const Emit &emit) {
    constexpr int NV = DIM + 1;
    const double *g = a.geo + e * a.geoStride;
    double gl[NV][DIM];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int d = 0; d < DIM; ++d) gl[k][d] = g[k * DIM + d];
    elem_forces_bilinear<DIM, DEG, MAT, SHIFT>(g, g[12], gl, gl, xl, emit, a.shift);
}

// ------------------------------------------------------------------------------------------------
// Discrete shape derivatives (forward mode): change of the element quantities under a perturbation delta_p of the
// mesh vertices, with the nodal fields held fixed (LinearElasticity.hh:238-330; Simulator level :1301-1374).
// Everything depends on the geometry through (grad lambda, vol) only:
//     delta grad lambda_i = - sum_k grad lambda_k (grad lambda_i . delta_p_k)      (EmbeddedElement.hh:269-278)
//     delta vol / vol     =   sum_k grad lambda_k . delta_p_k                       (EmbeddedElement.hh:366-372)
// and grad phi_i has the same (s,t) support form in delta grad lambda as in grad lambda (:338-363), so each
// derivative is the original kernel evaluated on perturbed gradients (product rule on the bilinear forms).
// ------------------------------------------------------------------------------------------------
template <int DIM>
DEV void load_corner_perturbation(const double *__restrict__ g, const int32_t *__restrict__ en /* element's nodes: corners first */,
                                  const double *__restrict__ deltaP, double (&gl)[DIM + 1][DIM], double (&dgl)[DIM + 1][DIM],
                                  double &relDeltaVol) {
    constexpr int NV = DIM + 1;
    double dp[NV][DIM];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int64_t v = en[k];
#pragma unroll
        for (int d = 0; d < DIM; ++d) { gl[k][d] = g[k * DIM + d]; dp[k][d] = deltaP[v * DIM + d]; dgl[k][d] = 0.0; }
    }
    relDeltaVol = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) relDeltaVol += gl[k][d] * dp[k][d];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            double sdot = 0;
#pragma unroll
            for (int d = 0; d < DIM; ++d) sdot += gl[i][d] * dp[k][d];
#pragma unroll
            for (int d = 0; d < DIM; ++d) dgl[i][d] -= gl[k][d] * sdot;
        }
    }
}

// flattened (tensor-shear) symmetrised gradient of the nodal field xl at quadrature point q, built on the gradients gl:
// sym(sum_i u_i (x) grad phi_i(x_q)); P2: grad phi_k = (4 lam_k - 1) gl_k, grad phi_(s,t) = 4 (lam_t gl_s + lam_s gl_t)
// (EmbeddedElement.hh:315-332) at the vertex-associated points lam_k(x_q) = c0 if k == q else c1.
// AT_VERTEX: evaluate at vertex q instead (lam_k = [k == q]), the nodal values of the degree-(DEG-1) strain interpolant
template <int DIM, int DEG, bool AT_VERTEX = false>
DEV void grad_u_at(const double (&xl)[(DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6)][DIM], const double (&gl)[DIM + 1][DIM],
                   int q, double (&G)[DIM][DIM]) {
    constexpr int NV = DIM + 1;
    constexpr double c0 = AT_VERTEX ? 1.0 : (DIM == 3 ? 0.58541019662496845446 : 2.0 / 3.0);
    constexpr double c1 = AT_VERTEX ? 0.0 : (DIM == 3 ? 0.13819660112501051518 : 1.0 / 6.0);
#pragma unroll
    for (int p = 0; p < DIM; ++p)
#pragma unroll
        for (int r = 0; r < DIM; ++r) G[p][r] = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double ck[DIM];
        if (DEG == 1) {
#pragma unroll
            for (int p = 0; p < DIM; ++p) ck[p] = xl[k][p];
        } else {
            const double lk = (k == q) ? c0 : c1;
#pragma unroll
            for (int p = 0; p < DIM; ++p) ck[p] = (4 * lk - 1) * xl[k][p];
#pragma unroll
            for (int o = 0; o < NV; ++o)
                if (o != k) {
                    const double lo = (o == q) ? c0 : c1;
#pragma unroll
                    for (int p = 0; p < DIM; ++p) ck[p] += 4 * lo * xl[(DEG == 1 ? 0 : NV + edge_between<DIM>(k, o))][p];
                }
        }
#pragma unroll
        for (int p = 0; p < DIM; ++p)
#pragma unroll
            for (int r = 0; r < DIM; ++r) G[p][r] += ck[p] * gl[k][r];
    }
}

template <int DIM, int DEG>
DEV void sym_grad_u_at(const double (&xl)[(DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6)][DIM], const double (&gl)[DIM + 1][DIM],
                       int q, double (&ef)[DIM * (DIM + 1) / 2]) {
    double G[DIM][DIM];
    grad_u_at<DIM, DEG>(xl, gl, q, G);
#pragma unroll
    for (int p = 0; p < DIM; ++p)
#pragma unroll
        for (int r = p; r < DIM; ++r) ef[flat_idx<DIM>(p, r)] = 0.5 * (G[p][r] + G[r][p]);
}

// element prologue of k_strain_field and the stress-measure kernels: the element's barycentric gradients and its nodal values of uNodes
template <int DIM, int DEG>
DEV void load_elem_field(const LoadArgs &a, int64_t e, const double *__restrict__ uNodes, double (&gl)[DIM + 1][DIM],
                         double (&xl)[(DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6)][DIM]) {
    constexpr int NV = DIM + 1;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    const double *g = a.geo + e * a.geoStride;
    const int32_t *en = a.elemNodes + e * NPE;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int d = 0; d < DIM; ++d) gl[k][d] = g[k * DIM + d];
#pragma unroll
    for (int j = 0; j < NPE; ++j) {
        const int64_t node = en[j];
#pragma unroll
        for (int d = 0; d < DIM; ++d) xl[j][d] = uNodes[node * DIM + d];
    }
}

// flattened (tensor-shear) strain of the element's field at corner q, or the stress C : strain of the element record g
template <int DIM, int DEG, int MAT>
DEV void corner_tensor(const double *__restrict__ g, const double (&xl)[(DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6)][DIM],
                       const double (&gl)[DIM + 1][DIM], int q, int wantStress, double (&ef)[DIM * (DIM + 1) / 2]) {
    constexpr int FL = DIM * (DIM + 1) / 2;
    double G[DIM][DIM];
    grad_u_at<DIM, DEG, true>(xl, gl, q, G);
#pragma unroll
    for (int p = 0; p < DIM; ++p)
#pragma unroll
        for (int r = p; r < DIM; ++r) ef[flat_idx<DIM>(p, r)] = 0.5 * (G[p][r] + G[r][p]);
    if (wantStress) {
        double sd[FL], sg[FL];
#pragma unroll
        for (int c = 0; c < FL; ++c) sd[c] = ef[c] * (c < DIM ? 1.0 : 2.0);
        elem_D_apply<DIM, MAT>(g, sd, sg);
#pragma unroll
        for (int c = 0; c < FL; ++c) ef[c] = sg[c];
    }
}

// Strain (or stress) field as per-element interpolants (Simulator::strainField / stressField, LinearElasticity.hh:511-526;
// Element::strain :99-117): the nodal values of the degree-(DEG-1) interpolant, i.e. one value per element for P1 and the
// values at the NV corners for P2. out: [nElem][NQ][flatLen].
template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_strain_field(LoadArgs a, const double *__restrict__ uNodes, int wantStress, double *__restrict__ out) {
    constexpr int NV = DIM + 1;
    constexpr int FL = DIM * (DIM + 1) / 2;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr int NQ = DEG == 1 ? 1 : NV;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.nElem; e += (int64_t)gridDim.x * 256) {
        const double *g = a.geo + e * a.geoStride;
        double gl[NV][DIM], xl[NPE][DIM];
        load_elem_field<DIM, DEG>(a, e, uNodes, gl, xl);
        for (int q = 0; q < NQ; ++q) {
            double ef[FL];
            corner_tensor<DIM, DEG, MAT>(g, xl, gl, q, wantStress, ef);
#pragma unroll
            for (int c = 0; c < FL; ++c) out[(e * NQ + q) * FL + c] = ef[c];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Stress measures (VonMises.hh, SymmetricMatrix.hh eigenvalues / eigenDecomposition, FieldPostProcessing.hh vertexAveragedField).
// Everything per tensor lives in registers: every array below is indexed by unrolled compile-time constants only.
// ------------------------------------------------------------------------------------------------
constexpr int SM_VON_MISES = 1, SM_EIGENVALUES = 2, SM_EIGENVECTORS = 4;   // MFH_MEASURE_* of the C ABI

// One Jacobi rotation in the (p, q) plane of a symmetric 3x3 matrix, annihilating a_pq; r is the third index. The columns p, q of the
// accumulated rotations (v_kp, v_kq) follow when VEC. |theta| = inf (a_pq denormal against the diagonal gap) gives t = 0: the identity.
template <bool VEC>
DEV void jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p, double &v1q,
                       double &v2p, double &v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    if (VEC) {
        const double w0p = c * v0p - s * v0q, w0q = s * v0p + c * v0q;
        const double w1p = c * v1p - s * v1q, w1q = s * v1p + c * v1q;
        const double w2p = c * v2p - s * v2q, w2q = s * v2p + c * v2q;
        v0p = w0p; v0q = w0q; v1p = w1p; v1q = w1q; v2p = w2p; v2q = w2q;
    }
}

// order (la, column a) before (lb, column b)
template <bool VEC>
DEV void eig_cswap(double &la, double &lb, double &v0a, double &v0b, double &v1a, double &v1b, double &v2a, double &v2b) {
    if (lb < la) {
        double t = la; la = lb; lb = t;
        if (VEC) {
            t = v0a; v0a = v0b; v0b = t;
            t = v1a; v1a = v1b; v1b = t;
            t = v2a; v2a = v2b; v2b = t;
        }
    }
}

// s: flattened symmetric matrix in flat_idx order, TENSOR shear entries (what k_strain_field writes).
//   vm   the von Mises scalar sqrt(|vonMisesExtractor<N>() : s|_F^2): 3D sqrt(3/2 dev s : dev s); 2D the plane-stress value
//        sqrt(s00^2 + s11^2 - s00 s11 + 3 s01^2) (VonMises.hh:10-46), written as half a sum of squares so that nothing cancels
//   lam  eigenvalues, ascending (SelfAdjointEigenSolver's order); V[i][k] = component i of the unit eigenvector of lam[k]
// The matrix is divided by its largest |entry| first (entries near 1e+-150 neither overflow nor flush in the squares); a NaN entry makes
// every output NaN. 3D: cyclic Jacobi on named scalars, pairs (0,1) (0,2) (1,2) per sweep, until the off-diagonal part is below 1e-20 of
// the largest entry (quadratic convergence: a handful of sweeps; the closed trigonometric form loses digits near repeated eigenvalues).
// 2D: mean -+ hypot(half difference, shear).
template <int DIM, bool EIG, bool VEC>
DEV void sym_measures(const double (&s)[DIM * (DIM + 1) / 2], double &vm, double (&lam)[DIM], double (&V)[DIM][DIM]) {
    constexpr int FL = DIM * (DIM + 1) / 2;
    double m = 0.0;
#pragma unroll
    for (int c = 0; c < FL; ++c) m = fmax(m, fabs(s[c]));
    if (!(m > 0.0)) m = 1.0;            // the zero matrix (fmax skips NaN entries: they pass through the division below)
    double a[FL];
#pragma unroll
    for (int c = 0; c < FL; ++c) a[c] = s[c] / m;
    if constexpr (DIM == 3) {
        const double d01 = a[0] - a[1], d12 = a[1] - a[2], d20 = a[2] - a[0];
        vm = m * sqrt(0.5 * (d01 * d01 + d12 * d12 + d20 * d20) + 3.0 * (a[3] * a[3] + a[4] * a[4] + a[5] * a[5]));
        if (!EIG) return;
        double a00 = a[0], a11 = a[1], a22 = a[2], a12 = a[3], a02 = a[4], a01 = a[5];
        double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
        for (int sweep = 0; sweep < 16; ++sweep) {
            if (fabs(a01) + fabs(a02) + fabs(a12) <= 1e-20) break;      // (a NaN never passes: it spreads to every output)
            jacobi_rotate<VEC>(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            jacobi_rotate<VEC>(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            jacobi_rotate<VEC>(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        eig_cswap<VEC>(a00, a11, v00, v01, v10, v11, v20, v21);
        eig_cswap<VEC>(a11, a22, v01, v02, v11, v12, v21, v22);
        eig_cswap<VEC>(a00, a11, v00, v01, v10, v11, v20, v21);
        lam[0] = m * a00; lam[1] = m * a11; lam[2] = m * a22;
        if (VEC) {
            V[0][0] = v00; V[0][1] = v01; V[0][2] = v02;
            V[1][0] = v10; V[1][1] = v11; V[1][2] = v12;
            V[2][0] = v20; V[2][1] = v21; V[2][2] = v22;
        }
    } else {
        const double dd = a[0] - a[1];
        vm = m * sqrt(0.5 * (dd * dd + a[0] * a[0] + a[1] * a[1]) + 3.0 * a[2] * a[2]);
        if (!EIG) return;
        const double mean = 0.5 * a[0] + 0.5 * a[1], d = 0.5 * dd, r = hypot(d, a[2]);
        lam[0] = m * (mean - r);
        lam[1] = m * (mean + r);
        if (VEC) {
            // (A - lam1 I) v = 0 from the row with the larger pivot: v = (d + r, s01) for d >= 0, (s01, r - d) otherwise
            double x = d >= 0.0 ? d + r : a[2], y = d >= 0.0 ? a[2] : r - d;
            const double n = hypot(x, y);
            if (n > 0.0) { x /= n; y /= n; } else if (n == 0.0) { x = 0.0; y = 1.0; }
            V[0][1] = x; V[1][1] = y;
            V[0][0] = y; V[1][0] = -x;
        }
    }
}

// the requested measures of tensor i: vm[i], eval[i][DIM], evec[i][DIM][DIM] (row-major, eigenvector k in column k)
template <int DIM>
DEV void store_measures(const double (&s)[DIM * (DIM + 1) / 2], int what, int64_t i, double *__restrict__ vm, double *__restrict__ eval,
                        double *__restrict__ evec) {
    double v, lam[DIM], V[DIM][DIM];
    if (what & SM_EIGENVECTORS) sym_measures<DIM, true, true>(s, v, lam, V);
    else if (what & SM_EIGENVALUES) sym_measures<DIM, true, false>(s, v, lam, V);
    else sym_measures<DIM, false, false>(s, v, lam, V);
    if (what & SM_VON_MISES) vm[i] = v;
    if (what & SM_EIGENVALUES) {
#pragma unroll
        for (int k = 0; k < DIM; ++k) eval[i * DIM + k] = lam[k];
    }
    if (what & SM_EIGENVECTORS) {
#pragma unroll
        for (int r = 0; r < DIM; ++r)
#pragma unroll
            for (int k = 0; k < DIM; ++k) evec[(i * DIM + r) * DIM + k] = V[r][k];
    }
}

// measures of a caller's field of n flattened symmetric matrices: [n][flatLen]
template <int DIM>
__global__ void __launch_bounds__(256) k_sym_measures(int64_t n, const double *__restrict__ field, int what, double *__restrict__ vm,
                                                     double *__restrict__ eval, double *__restrict__ evec) {
    constexpr int FL = DIM * (DIM + 1) / 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double s[FL];
#pragma unroll
        for (int c = 0; c < FL; ++c) s[c] = field[i * FL + c];
        store_measures<DIM>(s, what, i, vm, eval, evec);
    }
}

// the same measures of the strain (stress) of the nodal displacements uNodes at the corners k_strain_field evaluates, fused: the tensor
// is never written. vm: [nElem][NQ], eval: [nElem][NQ][DIM], evec: [nElem][NQ][DIM][DIM].
template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_stress_measures(LoadArgs a, const double *__restrict__ uNodes, int wantStress, int what,
                                                        double *__restrict__ vm, double *__restrict__ eval, double *__restrict__ evec) {
    constexpr int NV = DIM + 1;
    constexpr int FL = DIM * (DIM + 1) / 2;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr int NQ = DEG == 1 ? 1 : NV;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.nElem; e += (int64_t)gridDim.x * 256) {
        const double *g = a.geo + e * a.geoStride;
        double gl[NV][DIM], xl[NPE][DIM];
        load_elem_field<DIM, DEG>(a, e, uNodes, gl, xl);
        for (int q = 0; q < NQ; ++q) {
            double ef[FL];
            corner_tensor<DIM, DEG, MAT>(g, xl, gl, q, wantStress, ef);
            store_measures<DIM>(ef, what, e * NQ + q, vm, eval, evec);
        }
    }
}

// Peak von Mises value over all corners with its flat corner index. The order is total, so the reduction gives the same pair in any
// grouping: a NaN comes before every number, then the larger value, and among equals the lower index.
DEV bool peak_before(double va, int64_t ia, double vb, int64_t ib) {
    const bool na = va != va, nb = vb != vb;
    if (na || nb) return na && (!nb || ia < ib);
    return va > vb || (va == vb && ia < ib);
}
// workgroup-wide (256 lanes) reduction of (v, i) pairs; the result is valid in thread 0. lds: 4 values + 4 indices
DEV void peak_block_reduce(double &v, int64_t &i, double *ldsV, long long *ldsI) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off, 64);
        const long long oi = __shfl_down((long long)i, off, 64);
        if (peak_before(ov, oi, v, i)) { v = ov; i = oi; }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { ldsV[w] = v; ldsI[w] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (peak_before(ldsV[k], ldsI[k], v, i)) { v = ldsV[k]; i = ldsI[k]; }
    }
}
constexpr long long PEAK_NO_INDEX = 0x7fffffffffffffffLL;

// first stage: one (value, index) pair per workgroup, partV / partI: [gridDim.x]
template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_peak_von_mises(LoadArgs a, const double *__restrict__ uNodes, int wantStress, double *__restrict__ partV,
                                                       long long *__restrict__ partI) {
    constexpr int NV = DIM + 1;
    constexpr int FL = DIM * (DIM + 1) / 2;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr int NQ = DEG == 1 ? 1 : NV;
    __shared__ double ldsV[4];
    __shared__ long long ldsI[4];
    double best = -HUGE_VAL;
    int64_t bestI = PEAK_NO_INDEX;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.nElem; e += (int64_t)gridDim.x * 256) {
        const double *g = a.geo + e * a.geoStride;
        double gl[NV][DIM], xl[NPE][DIM];
        load_elem_field<DIM, DEG>(a, e, uNodes, gl, xl);
        for (int q = 0; q < NQ; ++q) {
            double ef[FL], v, lam[DIM], V[DIM][DIM];
            corner_tensor<DIM, DEG, MAT>(g, xl, gl, q, wantStress, ef);
            sym_measures<DIM, false, false>(ef, v, lam, V);
            if (peak_before(v, e * NQ + q, best, bestI)) { best = v; bestI = e * NQ + q; }
        }
    }
    peak_block_reduce(best, bestI, ldsV, ldsI);
    if (threadIdx.x == 0) { partV[blockIdx.x] = best; partI[blockIdx.x] = bestI; }
}

// second stage: one workgroup over the partials
__global__ void __launch_bounds__(256) k_peak_finish(int nPart, const double *__restrict__ partV, const long long *__restrict__ partI,
                                                    double *__restrict__ outV, long long *__restrict__ outI) {
    __shared__ double ldsV[4];
    __shared__ long long ldsI[4];
    double best = -HUGE_VAL;
    int64_t bestI = PEAK_NO_INDEX;
    for (int k = threadIdx.x; k < nPart; k += 256)
        if (peak_before(partV[k], partI[k], best, bestI)) { best = partV[k]; bestI = partI[k]; }
    peak_block_reduce(best, bestI, ldsV, ldsI);
    if (threadIdx.x == 0) { outV[0] = best; outI[0] = bestI; }
}

// first stage over a plain array: the (value, index) pair of every workgroup by peak_before's order, for k_peak_finish
__global__ void __launch_bounds__(256) k_peak_of_array(int64_t n, const double *__restrict__ v, double *__restrict__ partV, long long *__restrict__ partI) {
    __shared__ double ldsV[4];
    __shared__ long long ldsI[4];
    double best = -HUGE_VAL;
    int64_t bestI = PEAK_NO_INDEX;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double x = v[i];
        if (peak_before(x, i, best, bestI)) { best = x; bestI = i; }
    }
    peak_block_reduce(best, bestI, ldsV, ldsI);
    if (threadIdx.x == 0) { partV[blockIdx.x] = best; partI[blockIdx.x] = bestI; }
}

// ------------------------------------------------------------------------------------------------
// Modal stress recovery (mfh_modal_quadratic_stress, mfh_modal_random_stress; docs/design/04_24_modal_stress.md): per element corner the
// sums over np <= 32 displacement planes u_t (VARIABLE numbering, ldu apart; the node -> DoF table of a.dofForNode, identity if null) of
//     comp[e][q][c] += s_c(u_t)^2,   vm[e][q] += v2(s(u_t)),   s = corner_tensor's strain or stress of plane t at corner q,
// t ascending: accC = fma(s_c, s_c, accC), accV += v2. v2 is the square of sym_measures' von Mises scalar WITHOUT its division by the
// largest entry (the sums over the planes must be absolute): half a sum of squares, every term >= 0, nothing cancels. So the squares
// have to stay inside the double range, as for k_modal_sumsq. One lane per element; the element record (gradients, material) stays in
// registers over the planes; the accumulators start from 0.0 (first) or from the outputs, and are stored as they are or, under root,
// as their square roots: neither the pass boundaries nor the planes per pass change a bit. No LDS, no atomics; planes beyond np are
// not read. comp may be null.
template <int DIM>
DEV double von_mises_sq(const double (&s)[DIM * (DIM + 1) / 2]) {
    if constexpr (DIM == 3) {
        const double d01 = s[0] - s[1], d12 = s[1] - s[2], d20 = s[2] - s[0];
        return 0.5 * (d01 * d01 + d12 * d12 + d20 * d20) + 3.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]);
    } else {
        const double dd = s[0] - s[1];
        return 0.5 * (dd * dd + s[0] * s[0] + s[1] * s[1]) + 3.0 * s[2] * s[2];
    }
}

template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_modal_stress_sumsq(LoadArgs a, const double *__restrict__ U, int64_t ldu, int np, int wantStress, int first, int root,
                                                           double *__restrict__ vm, double *__restrict__ comp) {
    constexpr int NV = DIM + 1;
    constexpr int FL = DIM * (DIM + 1) / 2;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr int NQ = DEG == 1 ? 1 : NV;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.nElem; e += (int64_t)gridDim.x * 256) {
        const double *g = a.geo + e * a.geoStride;
        const int32_t *en = a.elemNodes + e * NPE;
        double gl[NV][DIM];
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int d = 0; d < DIM; ++d) gl[k][d] = g[k * DIM + d];
        int64_t var[NPE];           // first variable of every node
#pragma unroll
        for (int j = 0; j < NPE; ++j) {
            const int32_t node = en[j];
            var[j] = (int64_t)(a.dofForNode ? a.dofForNode[node] : node) * DIM;
        }
        double accV[NQ], accC[NQ][FL];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            accV[q] = first ? 0.0 : vm[e * NQ + q];
#pragma unroll
            for (int c = 0; c < FL; ++c) accC[q][c] = (first || !comp) ? 0.0 : comp[(e * NQ + q) * FL + c];
        }
        for (int t = 0; t < np; ++t) {
            const double *__restrict__ u = U + (int64_t)t * ldu;
            double xl[NPE][DIM];
#pragma unroll
            for (int j = 0; j < NPE; ++j)
#pragma unroll
                for (int d = 0; d < DIM; ++d) xl[j][d] = u[var[j] + d];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                double ef[FL];
                corner_tensor<DIM, DEG, MAT>(g, xl, gl, q, wantStress, ef);
#pragma unroll
                for (int c = 0; c < FL; ++c) accC[q][c] = fma(ef[c], ef[c], accC[q][c]);
                accV[q] += von_mises_sq<DIM>(ef);
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            vm[e * NQ + q] = root ? sqrt(accV[q]) : accV[q];
            if (comp) {
#pragma unroll
                for (int c = 0; c < FL; ++c) comp[(e * NQ + q) * FL + c] = root ? sqrt(accC[q][c]) : accC[q][c];
            }
        }
    }
}

// C0 volume-weighted vertex average of per-element corner values (vertexAveragedField, FieldPostProcessing.hh:24-47): one lane per
// vertex walks the vertex's (element, local node) pairs of the node-pair list (ascending by element, code = e npe + j) and accumulates
// vol_e value and vol_e in that order; nothing is added atomically. field: [nElem][nq][C] with nq = 1 (every corner takes the element's
// value) or NV; this launch averages the CB components [c0, c0 + CB). A vertex of a single element takes that element's value as it is;
// pairs with j >= NV (a caller-numbered quadratic mesh, where every node counts as a vertex) are no corners: such a node gets 0.
template <int CB>
__global__ void __launch_bounds__(256) k_vertex_average(int64_t nVert, const int32_t *__restrict__ nodePtr, const int32_t *__restrict__ nodePair,
                                                       int npe, int NV, const double *__restrict__ geo, int geoStride,
                                                       const double *__restrict__ field, int nq, int C, int c0, double *__restrict__ out) {
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < nVert; n += (int64_t)gridDim.x * 256) {
        const int first = nodePtr[n], last = nodePtr[n + 1];
        double acc[CB], w = 0.0;
#pragma unroll
        for (int k = 0; k < CB; ++k) acc[k] = 0.0;
        int corners = 0;
        for (int p = first; p < last; ++p) {
            const int64_t code = nodePair[p], e = code / npe;
            const int j = (int)(code - e * npe);
            if (j >= NV) continue;
            const double *f = field + (e * nq + (nq == 1 ? 0 : j)) * C + c0;
            if (last - first == 1) {
#pragma unroll
                for (int k = 0; k < CB; ++k) acc[k] = f[k];
                w = 1.0;
            } else {
                const double vol = geo[e * geoStride + 12];
#pragma unroll
                for (int k = 0; k < CB; ++k) acc[k] += vol * f[k];
                w += vol;
            }
            ++corners;
        }
#pragma unroll
        for (int k = 0; k < CB; ++k) out[n * C + c0 + k] = corners == 0 ? 0.0 : (last - first == 1 ? acc[k] : acc[k] / w);
    }
}

// The strain (stress) interpolant of the parent element restricted to every boundary element (restrictInterpolant,
// InterpolantRestriction.hh:29-66, applied to Element::strain): the nodal values of the degree-(DEG-1) interpolant on the
// boundary simplex, i.e. one value for P1 and the values at the boundary element's DIM corners (in its own vertex order)
// for P2. One thread per boundary element; the corner is located in the parent by its node id. out: [nBE][1 | DIM][flatLen].
template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_boundary_strain_field(LoadArgs a, int64_t nBE, const int32_t *__restrict__ bdryParent,
                                                               const int32_t *__restrict__ bdryElemNodes, int npbe,
                                                               const double *__restrict__ uNodes, int wantStress, double *__restrict__ out) {
    constexpr int NV = DIM + 1;
    constexpr int FL = DIM * (DIM + 1) / 2;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr int NQ = DEG == 1 ? 1 : DIM;
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < nBE; b += (int64_t)gridDim.x * 256) {
        const int64_t e = bdryParent[b];
        const double *g = a.geo + e * a.geoStride;
        const int32_t *en = a.elemNodes + e * NPE;
        double gl[NV][DIM], xl[NPE][DIM];
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int d = 0; d < DIM; ++d) gl[k][d] = g[k * DIM + d];
#pragma unroll
        for (int j = 0; j < NPE; ++j) {
            const int64_t node = en[j];
#pragma unroll
            for (int d = 0; d < DIM; ++d) xl[j][d] = uNodes[node * DIM + d];
        }
        for (int c = 0; c < NQ; ++c) {
            int q = 0;
            if (DEG == 2) {
                const int32_t corner = bdryElemNodes[b * npbe + c];
#pragma unroll
                for (int k = 0; k < NV; ++k)
                    if (en[k] == corner) q = k;
            }
            double G[DIM][DIM], ef[FL];
            grad_u_at<DIM, DEG, true>(xl, gl, q, G);
#pragma unroll
            for (int p = 0; p < DIM; ++p)
#pragma unroll
                for (int r = p; r < DIM; ++r) ef[flat_idx<DIM>(p, r)] = 0.5 * (G[p][r] + G[r][p]);
            if (wantStress) {
                double sd[FL], sg[FL];
#pragma unroll
                for (int i = 0; i < FL; ++i) sd[i] = ef[i] * (i < DIM ? 1.0 : 2.0);
                elem_D_apply<DIM, MAT>(g, sd, sg);
#pragma unroll
                for (int i = 0; i < FL; ++i) ef[i] = sg[i];
            }
#pragma unroll
            for (int i = 0; i < FL; ++i) out[(b * NQ + c) * FL + i] = ef[i];
        }
    }
}

// The exact differential of the mutual energies with respect to every vertex coordinate
// (homogenizedElasticityTensorDiscreteDifferential, PeriodicHomogenization.hh:372-480, before the division by |Y|):
// for the unit perturbation e_c of vertex v, delta vol / vol = gl_v[c] and delta grad lambda_i = -gl_v gl_i[c], so that
// (delta eps)(w) = -sym(grad w[:, c] (x) gl_v) and the element's contribution to d/dp_v is  Q gl_v  with the
// Eshelby-like tensor
//     Q = int (G^ij : S^kl) I - (grad w^ij)^T S^kl - (grad w^kl)^T S^ij dV,     S = C : G, G = e + eps(w).
// One workgroup column per tensor entry ij <= kl (blockIdx.y); out: [pair][nVert][DIM], atomics per element corner.
template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_mutual_energy_differential(LoadArgs a, const double *__restrict__ w, int64_t nNode,
                                                                    int64_t nVert, double *__restrict__ out) {
    constexpr int NV = DIM + 1;
    constexpr int FL = DIM * (DIM + 1) / 2;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr int NQ = DEG == 1 ? 1 : NV;
    int ij = 0, rem = blockIdx.y;
    while (rem >= FL - ij) { rem -= FL - ij; ++ij; }
    const int kl = ij + rem;
    const double *wij = w + (int64_t)ij * nNode * DIM, *wkl = w + (int64_t)kl * nNode * DIM;
    double *o = out + (int64_t)blockIdx.y * nVert * DIM;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.nElem; e += (int64_t)gridDim.x * 256) {
        const double *g = a.geo + e * a.geoStride;
        const int32_t *en = a.elemNodes + e * NPE;
        double gl[NV][DIM];
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int d = 0; d < DIM; ++d) gl[k][d] = g[k * DIM + d];
        double xa[NPE][DIM], xb[NPE][DIM];
#pragma unroll
        for (int j = 0; j < NPE; ++j) {
            const int64_t node = en[j];
#pragma unroll
            for (int d = 0; d < DIM; ++d) { xa[j][d] = wij[node * DIM + d]; xb[j][d] = wkl[node * DIM + d]; }
        }
        double Q[DIM][DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c)
#pragma unroll
            for (int r = 0; r < DIM; ++r) Q[c][r] = 0.0;
        for (int q = 0; q < NQ; ++q) {
            double Wa[DIM][DIM], Wb[DIM][DIM], Ga[FL], Gb[FL], Sa[FL], Sb[FL], sd[FL];
            grad_u_at<DIM, DEG>(xa, gl, q, Wa);
            grad_u_at<DIM, DEG>(xb, gl, q, Wb);
#pragma unroll
            for (int p = 0; p < DIM; ++p)
#pragma unroll
                for (int r = p; r < DIM; ++r) {
                    const int c = flat_idx<DIM>(p, r);
                    Ga[c] = 0.5 * (Wa[p][r] + Wa[r][p]) + ((c == ij) ? (c < DIM ? 1.0 : 0.5) : 0.0);
                    Gb[c] = 0.5 * (Wb[p][r] + Wb[r][p]) + ((c == kl) ? (c < DIM ? 1.0 : 0.5) : 0.0);
                }
#pragma unroll
            for (int c = 0; c < FL; ++c) sd[c] = Ga[c] * (c < DIM ? 1.0 : 2.0);
            elem_D_apply<DIM, MAT>(g, sd, Sa);
#pragma unroll
            for (int c = 0; c < FL; ++c) sd[c] = Gb[c] * (c < DIM ? 1.0 : 2.0);
            elem_D_apply<DIM, MAT>(g, sd, Sb);
            double E = 0.0;
#pragma unroll
            for (int c = 0; c < FL; ++c) E += (c < DIM ? 1.0 : 2.0) * Ga[c] * Sb[c];
#pragma unroll
            for (int c = 0; c < DIM; ++c)
#pragma unroll
                for (int r = 0; r < DIM; ++r) {
                    double t = 0.0;
#pragma unroll
                    for (int p = 0; p < DIM; ++p) t += Wa[p][c] * Sb[flat_idx<DIM>(p, r)] + Wb[p][c] * Sa[flat_idx<DIM>(p, r)];
                    Q[c][r] += ((c == r) ? E : 0.0) - t;
                }
        }
        const double sc = g[12] / NQ;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int64_t v = en[k];
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                double val = 0.0;
#pragma unroll
                for (int r = 0; r < DIM; ++r) val += Q[c][r] * gl[k][r];
                unsafeAtomicAdd(&o[v * DIM + c], sc * val);
            }
        }
    }
}

// Mutual energies of the cell-problem fields, sum_e int (e^ij + eps(w^ij)) : C : (e^kl + eps(w^kl)) dV for every pair
// ij <= kl (blockIdx.y), i.e. |Y| Ch in the energy form (PeriodicHomogenization.hh:146-186 without the averaging
// shortcut), and with deltaP their discrete shape derivative in the volume form quoted at
// PeriodicHomogenization.hh:484-491:  int rel G^ij:C:G^kl + (delta eps)(w^ij):C:G^kl + G^ij:C:(delta eps)(w^kl) dV
// (the terms in delta w vanish by the cell problems' stationarity). w: [flatLen][nNode][DIM] per-node fields.
template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_mutual_energies(LoadArgs a, const double *__restrict__ w, int64_t nNode,
                                                         const double *__restrict__ deltaP, double *__restrict__ out) {
    constexpr int NV = DIM + 1;
    constexpr int FL = DIM * (DIM + 1) / 2;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr int NQ = DEG == 1 ? 1 : NV;
    // pair index -> (ij, kl), ij <= kl, row-major over the upper triangle
    int ij = 0, rem = blockIdx.y;
    while (rem >= FL - ij) { rem -= FL - ij; ++ij; }
    const int kl = ij + rem;
    const double *wij = w + (int64_t)ij * nNode * DIM, *wkl = w + (int64_t)kl * nNode * DIM;
    double acc = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.nElem; e += (int64_t)gridDim.x * 256) {
        const double *g = a.geo + e * a.geoStride;
        const int32_t *en = a.elemNodes + e * NPE;
        double gl[NV][DIM], dgl[NV][DIM], rel = 0.0;
        if (deltaP) load_corner_perturbation<DIM>(g, en, deltaP, gl, dgl, rel);
        else {
#pragma unroll
            for (int k = 0; k < NV; ++k)
#pragma unroll
                for (int d = 0; d < DIM; ++d) gl[k][d] = g[k * DIM + d];
        }
        double xa[NPE][DIM], xb[NPE][DIM];
#pragma unroll
        for (int j = 0; j < NPE; ++j) {
            const int64_t node = en[j];
#pragma unroll
            for (int d = 0; d < DIM; ++d) { xa[j][d] = wij[node * DIM + d]; xb[j][d] = wkl[node * DIM + d]; }
        }
        double sum = 0.0;
        for (int q = 0; q < NQ; ++q) {
            double Ga[FL], Gb[FL], Sa[FL], Sb[FL], sd[FL];
            sym_grad_u_at<DIM, DEG>(xa, gl, q, Ga);
            sym_grad_u_at<DIM, DEG>(xb, gl, q, Gb);
#pragma unroll
            for (int c = 0; c < FL; ++c) {   // + canonical basis strains (SymmetricMatrix.hh:405-413)
                Ga[c] += (c == ij) ? (c < DIM ? 1.0 : 0.5) : 0.0;
                Gb[c] += (c == kl) ? (c < DIM ? 1.0 : 0.5) : 0.0;
            }
#pragma unroll
            for (int c = 0; c < FL; ++c) sd[c] = Gb[c] * (c < DIM ? 1.0 : 2.0);
            elem_D_apply<DIM, MAT>(g, sd, Sb);
            if (deltaP) {
                double dA[FL], dB[FL];
                sym_grad_u_at<DIM, DEG>(xa, dgl, q, dA);
                sym_grad_u_at<DIM, DEG>(xb, dgl, q, dB);
#pragma unroll
                for (int c = 0; c < FL; ++c) sd[c] = Ga[c] * (c < DIM ? 1.0 : 2.0);
                elem_D_apply<DIM, MAT>(g, sd, Sa);
#pragma unroll
                for (int c = 0; c < FL; ++c) {
                    const double m = c < DIM ? 1.0 : 2.0;
                    sum += m * ((rel * Ga[c] + dA[c]) * Sb[c] + dB[c] * Sa[c]);
                }
            } else {
#pragma unroll
                for (int c = 0; c < FL; ++c) sum += (c < DIM ? 1.0 : 2.0) * Ga[c] * Sb[c];
            }
        }
        acc += sum * g[12] / NQ;
    }
    // wave reduction, one atomic per wave
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(&out[blockIdx.y], acc);
}

// (delta K) u, Simulator::applyDeltaStiffnessMatrix (LinearElasticity.hh:1301-1328) with deltaPerElementStiffness
// (:306-330) never formed: delta f = vol [B(rel gl + dgl, gl) + B(gl, dgl)] u with B the bilinear form above
// (rel = delta vol / vol). u is a per-NODE field, the result a per-DoF field, exactly as in the reference.
template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_apply_delta_K(LoadArgs a, const double *__restrict__ uNodes, const double *__restrict__ deltaP,
                                                       double *__restrict__ out) {
    constexpr int NV = DIM + 1;
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.nElem; e += (int64_t)gridDim.x * 256) {
        const double *g = a.geo + e * a.geoStride;
        const int32_t *en = a.elemNodes + e * NPE;
        double gl[NV][DIM], dgl[NV][DIM], glA[NV][DIM], rel;
        load_corner_perturbation<DIM>(g, en, deltaP, gl, dgl, rel);
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int d = 0; d < DIM; ++d) glA[k][d] = rel * gl[k][d] + dgl[k][d];
        double xl[NPE][DIM];
        int64_t dof[NPE];
#pragma unroll
        for (int j = 0; j < NPE; ++j) {
            const int64_t node = en[j];
            dof[j] = a.dofForNode ? (int64_t)a.dofForNode[node] : node;
#pragma unroll
            for (int d = 0; d < DIM; ++d) xl[j][d] = uNodes[node * DIM + d];
        }
        // first term kept in registers so that every (node, component) costs one atomic, not two
        double f1[NPE][DIM];
        elem_forces_bilinear<DIM, DEG, MAT>(g, g[12], glA, gl, xl, [&](int j, const double *fv) {
#pragma unroll
            for (int d = 0; d < DIM; ++d) f1[j][d] = fv[d];
        });
        elem_forces_bilinear<DIM, DEG, MAT>(g, g[12], gl, dgl, xl, [&](int j, const double *fv) {
#pragma unroll
            for (int d = 0; d < DIM; ++d) unsafeAtomicAdd(&out[dof[j] * DIM + d], f1[j][d] + fv[d]);
        });
    }
}

template <int DIM, int DEG, int MAT>
__global__ void __launch_bounds__(256) k_mf_forces(SpmvMfArgs a, const double *__restrict__ x, double *__restrict__ fbuf,
                                                   const double *scal, int it, const double *stopPtr) {
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    if (scal) {
        it += (int)stopPtr[3];
        if (scal[(int64_t)it * 4 + 2] <= stopPtr[0]) return;
    }
    const int64_t nE = a.nElem;
    // element groups of 256: XCD-contiguous ranges of groups, see xcd_span
    int64_t grpFirst = blockIdx.x, grpEnd = (nE + 255) / 256, grpStride = gridDim.x;
    if (a.xcd) xcd_span(grpEnd, grpFirst, grpEnd, grpStride);
    for (int64_t grp = grpFirst; grp < grpEnd; grp += grpStride) {
        const int64_t e = grp * 256 + threadIdx.x;
        if (e >= nE) continue;
        double f[NPE][DIM];
        elem_forces<DIM, DEG, MAT>(a, e, x, f);
        if (a.pairPos) {
            // list order: the pair's force goes where the rows pass will stream it
#pragma unroll
            for (int j = 0; j < NPE; ++j) {
                const uint32_t pp = a.pairPos[e * NPE + j];
                if (pp == 0xffffffffu) continue;
#pragma unroll
                for (int d = 0; d < DIM; ++d) fbuf[(int64_t)pp * DIM + d] = f[j][d];
            }
            continue;
        }
        // element-major AoS: the (element, node) pair with code e*NPE + i owns fbuf[code*DIM .. +DIM)
        double *o = fbuf + e * (NPE * DIM);
        if ((NPE * DIM) % 2 == 0) {
            typedef double dv2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int q = 0; q < NPE * DIM / 2; ++q) {
                dv2 w = {f[(2 * q) / DIM][(2 * q) % DIM], f[(2 * q + 1) / DIM][(2 * q + 1) % DIM]};
                *reinterpret_cast<dv2 *>(o + 2 * q) = w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < NPE * DIM; ++q) o[q] = f[q / DIM][q % DIM];
        }
    }
}

// Cluster variant: one workgroup per block of MF_BLOCK consecutive elements. The nodal forces of the block are summed
// in LDS (one accumulator per distinct row of the block). Rows whose elements all belong to the block are finished
// here and written to y; the other rows leave ONE partial sum per (block, row) in the interface buffer, in row order,
// which k_mf_rows sums. With a spatially coherent element order most rows are finished in their block, so the
// 240 B/element force buffer of k_mf_forces shrinks to a few tens of bytes per element.
// PCG: 0 = plain operator (optional dotOut), 1 = classic PCG bookkeeping (scal[it 4 + {1: p.Ap, 2: r.r}], base stopPtr[3],
// threshold stopPtr[0]), 2 = Chronopoulos-Gear bookkeeping for ONE right-hand side (delta into scal[(it + 1) 4 + 1], base
// ctl[0], threshold ctl[2]; see k_mf_cluster_nr). blockList (may be null = all blocks) selects the blocks of this launch.
// GEOV: the element's gradients and volume are RECOMPUTED from its four (three) corner positions instead of being read from
// its 128-byte record: the positions (24 B per vertex, shared by ~24 tets) stay in L2 / the memory-side cache, so a block of
// 256 P2 tets reads ~10 KB of connectivity instead of 32 KB of records from HBM, for ~80 more FP64 instructions per element.
// Only with a constant material (its part of the record is then the same for every element: element 0's is used).
template <int DIM, int DEG, int MAT, int PCG, bool GEOV = false, bool DET = false, bool SHIFT = false>
__global__ void __launch_bounds__(MF_BLOCK) k_mf_cluster(SpmvMfArgs a, const double *__restrict__ x, double *__restrict__ y, double *dotOut,
                                                         double *scal, int it, const double *stopPtr, const int32_t *__restrict__ blockList,
                                                         int64_t nList) {
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    extern __shared__ __attribute__((aligned(16))) double clacc[];   // accumulators [maxLocal * DIM] (x 4 when deterministic) + staged x [maxLocal * DIM] + 16
    // Option "deterministic": the order in which the four waves reach a shared accumulator changes from run to run, so every wave sums
    // into an array of its own (inside ONE wave the hardware applies the lanes of an LDS atomic in a fixed order) and the write-out adds
    // the four in wave order.
    // LDS layout of the staged x and of the accumulators: [row][DIM] (default) or, with -DMFH_XS_SOA (experiment: fewer bank conflicts
    // on the 8-byte gathers by local row index?), [DIM][row]
#ifdef MFH_XS_SOA
#define LIDX(t, d) ((d) * a.clMaxLocal + (t))
#else
#define LIDX(t, d) ((t) * DIM + (d))
#endif
    constexpr bool det = DET;          // = (a.det.partials != nullptr), chosen by the launcher: the default instantiation has one accumulator array
    const int accStride = a.clMaxLocal * DIM;
    double *xs = clacc + (det ? 4 : 1) * accStride;
    double *red = xs + accStride;
    double *accw = clacc + (det ? (int)(threadIdx.x >> 6) * accStride : 0);
    if (PCG == 1) {
        it += (int)stopPtr[3];
        if (scal[(int64_t)it * 4 + 2] <= stopPtr[0]) return;
        dotOut = scal + (int64_t)it * 4 + 1;
    } else if (PCG == 2) {
        it += (int)stopPtr[0];
        if (scal[(int64_t)it * 4 + 2] <= stopPtr[2]) return;
        dotOut = scal + (int64_t)(it + 1) * 4 + 1;
    }
    double dot = 0.0;
    for (int64_t q = blockIdx.x; q < nList; q += gridDim.x) {
        const int64_t b = blockList ? (int64_t)blockList[q] : (a.xcd > 1 ? xcd_group_item(q, nList, a.xcd) : q);
        const int u0 = a.clBlockPtr[b], nLocal = a.clBlockPtr[b + 1] - u0;
        // x of every distinct row of the block is read ONCE into LDS (a block of 256 P2 tets gathers 2560 nodal vectors
        // but touches only ~580 distinct rows); the lanes then pick their 10 vectors from LDS by local row index
        for (int t = threadIdx.x; t < nLocal; t += MF_BLOCK) {
            const int64_t row = a.clEntryRow[u0 + t];
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                xs[LIDX(t, d)] = SHIFT ? 0.0 : x[row * DIM + d]; clacc[LIDX(t, d)] = 0.0;    // (SHIFT: u = 0, the load of a constant strain)
                if (det) { clacc[accStride + LIDX(t, d)] = 0.0; clacc[2 * accStride + LIDX(t, d)] = 0.0; clacc[3 * accStride + LIDX(t, d)] = 0.0; }
            }
        }
        __syncthreads();
        // lane -> element of the block: with a stride coprime to the block size the lanes of a wave take elements that are
        // far apart in the block, so they rarely add to the SAME row at the same instruction (consecutive elements share
        // nodes -- the 24 tets of a generator hex all contain its centre vertex -- and same-address LDS atomics serialise)
        // blocks of whole cells (clElemPtr, <= MF_BLOCK elements each) or of clBlockElems consecutive elements
        const int64_t e0 = a.clElemPtr ? (int64_t)a.clElemPtr[b] : b * a.clBlockElems;
        const int ne = a.clElemPtr ? a.clElemPtr[b + 1] - a.clElemPtr[b] : a.clBlockElems;
        // A block may hold more elements than the workgroup has lanes (up to MF_BLOCK_ELEMS_MAX, round 5): the lanes take them in rounds of
        // MF_BLOCK -- the staging of x, the two barriers and the write-out of a block are then shared by twice the elements (operator 0.68 /
        // 0.47 ms at 128 / 256 elements per block).
        const int span = (a.clElemPtr || a.clBlockElems > MF_BLOCK) ? MF_BLOCK : a.clBlockElems;      // the lane permutation is a bijection of [0, span)
        const int le0 = a.clLaneStride > 1 ? (int)((threadIdx.x * (unsigned)a.clLaneStride) % (unsigned)span) : (int)threadIdx.x;
        for (int base = 0; base < ne; base += MF_BLOCK) {
        const int le = base + le0;
        const int64_t e = e0 + le;
        if ((int)threadIdx.x < span && le < ne && e < a.nElem) {
            int li[NPE];
            double xl[NPE][DIM];
#pragma unroll
            for (int j = 0; j < NPE; ++j) {
                li[j] = a.clLocalIdx[e * NPE + j];
#pragma unroll
                for (int d = 0; d < DIM; ++d) xl[j][d] = xs[LIDX(li[j], d)];
            }
            auto emit = [&](int j, const double *fv) {
#pragma unroll
                for (int d = 0; d < DIM; ++d) unsafeAtomicAdd(&accw[LIDX(li[j], d)], fv[d]);
            };
            if (GEOV) {
                const int32_t *en = a.elemNodes + e * NPE;
                double P[DIM + 1][DIM], gl[DIM + 1][DIM], vol;
#pragma unroll
                for (int k = 0; k <= DIM; ++k) {
                    const int64_t v = en[k];
#pragma unroll
                    for (int d = 0; d < DIM; ++d) P[k][d] = a.vertPos[v * DIM + d];
                }
                embed_simplex<DIM>(P, gl, vol);
                elem_forces_bilinear<DIM, DEG, MAT, SHIFT>(a.geo, vol, gl, gl, xl, emit, a.shift);
            } else
                elem_forces_core<DIM, DEG, MAT, SHIFT>(a, a.clElemPerm ? (int64_t)a.clElemPerm[e] : e, xl, emit);   // the record of the ORIGINAL element
        }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < nLocal; t += MF_BLOCK) {
            const int dest = a.clEntryDest[u0 + t];
            if (dest == -2) continue;                                  // row owned by another rank
            if (det) {
#pragma unroll
                for (int d = 0; d < DIM; ++d)
                    clacc[LIDX(t, d)] = ((clacc[LIDX(t, d)] + clacc[accStride + LIDX(t, d)]) + clacc[2 * accStride + LIDX(t, d)]) + clacc[3 * accStride + LIDX(t, d)];
            }
            if (dest >= 0) {
                // an interface row: the partial goes to the second pass. Inside a PCG loop its share of p . (K p) is taken HERE, where p is staged
                // (the inner product is linear in the partials), so that k_mf_rows needs no scattered read of p: 96 -> 59 us per iteration at
                // configs[2]. No look at the fixed-variable mask (a row index and three mask bytes fetched here cost the kernel 60 us: loads in
                // the write-out lengthen every block's critical path): a PCG's direction is zero on the fixed variables, so they add nothing.
                // Plain applications (any x) leave the interface rows' share to k_mf_rows, which has the mask.
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    const double v = clacc[LIDX(t, d)];
                    a.clIfaceBuf[(int64_t)dest * DIM + d] = v;
                    if (PCG != 0) dot += v * xs[LIDX(t, d)];
                }
                continue;
            }
            const int64_t row = a.clEntryRow[u0 + t];
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                const int64_t gi = row * DIM + d;
                double v = clacc[LIDX(t, d)];
                if (a.fixedMask && a.fixedMask[gi]) v = 0.0;
                y[gi] = v;
                if (dotOut) dot += v * xs[LIDX(t, d)];     // x of this row is still staged in LDS: no second (scattered) global read
            }
        }
        __syncthreads();
    }
    if (dotOut) {
        double v[1] = {dot};
        block_sum<1>(v, red);
        double *const tg[1] = {dotOut};
        commit_sums<1>(v, tg, a.det, red);
    }
}
#undef LIDX

// y_row = sum over the (element, node) pairs of the row of their nodal force: a pure gather-sum
template <int DIM, int PCG, bool DET = false>
__global__ void __launch_bounds__(256) k_mf_rows(SpmvMfArgs a, const double *__restrict__ fbuf, const double *__restrict__ x,
                                                 double *__restrict__ y, double *dotOut, double *scal, int it, const double *stopPtr) {
    extern __shared__ __attribute__((aligned(16))) double mfacc[];   // [maxRows * DIM] + 16
    double *red = mfacc + a.maxRows * DIM;
    if (PCG == 1) {
        it += (int)stopPtr[3];
        if (scal[(int64_t)it * 4 + 2] <= stopPtr[0]) return;
        dotOut = scal + (int64_t)it * 4 + 1;
    } else if (PCG == 2) {
        it += (int)stopPtr[0];
        if (scal[(int64_t)it * 4 + 2] <= stopPtr[2]) return;
        dotOut = scal + (int64_t)(it + 1) * 4 + 1;
    }
    double dot = 0.0;
    int64_t chunkFirst = blockIdx.x, chunkEnd = a.nChunk, chunkStride = gridDim.x;
    if (a.xcd) xcd_span(a.nChunk, chunkFirst, chunkEnd, chunkStride);
    for (int64_t chunk = chunkFirst; chunk < chunkEnd; chunk += chunkStride) {
        const int r0 = a.chunkRow[chunk], r1 = a.chunkRow[chunk + 1];
        const int nr = (r1 - r0) * DIM;
        for (int t = threadIdx.x; t < nr; t += 256) mfacc[t] = 0.0;
        __syncthreads();
        const int64_t kb = a.pairPtr[chunk], ke = a.pairPtr[chunk + 1];
        // U independent pairs per lane and trip: their list and force loads are all in flight together
        constexpr int U = 2;
        // (deterministic mode has barriers inside the loop: every lane runs the same number of trips)
        for (int64_t k0 = kb + threadIdx.x; DET ? (k0 - threadIdx.x < ke) : (k0 < ke); k0 += 256 * U) {
            int64_t code[U];
            int lr[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t kk = k0 + (int64_t)u * 256;
                ok[u] = kk < ke;
                code[u] = a.pairPos ? (ok[u] ? kk : kb) : (int64_t)(ok[u] ? a.pairCode[kk] : a.pairCode[kb]);
                lr[u] = ok[u] ? (int)a.pairRow[kk] : 0;
            }
            double out[U][DIM];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < DIM; ++c) out[u][c] = fbuf[code[u] * DIM + c];
            if (DET) {
                // option "deterministic" (DET = (a.det.partials != nullptr), chosen by the launcher): one wave after the other (a row's partials then meet in list order, whatever the timing)
                for (int w = 0; w < 4; ++w) {
                    if ((int)(threadIdx.x >> 6) == w) {
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            if (!ok[u]) continue;
#pragma unroll
                            for (int c = 0; c < DIM; ++c) unsafeAtomicAdd(&mfacc[lr[u] * DIM + c], out[u][c]);
                        }
                    }
                    __syncthreads();
                }
                continue;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
#pragma unroll
                for (int c = 0; c < DIM; ++c) unsafeAtomicAdd(&mfacc[lr[u] * DIM + c], out[u][c]);
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < nr; idx += 256) {
            int64_t gi = (int64_t)r0 * DIM + idx;
            if (a.rowMap) gi = (int64_t)a.rowMap[r0 + idx / DIM] * DIM + idx % DIM;   // cluster variant: compact numbering of the interface rows
            double v = mfacc[idx];
            if (a.fixedMask && a.fixedMask[gi]) v = 0.0;
            y[gi] = v;
            if (dotOut && !(PCG != 0 && a.rowMap)) dot += v * x[gi];          // (cluster variant inside a PCG loop: k_mf_cluster has taken the interface rows' share from its staged p)
        }
        __syncthreads();
    }
    if (dotOut && !(PCG != 0 && a.rowMap)) {
        double v[1] = {dot};
        block_sum<1>(v, red);
        double *const tg[1] = {dotOut};
        commit_sums<1>(v, tg, a.det, red);
    }
}

// ------------------------------------------------------------------------------------------------
// Operators of the batched / distributed PCG (mfh_solver.cpp). NR right-hand sides are interleaved per row: vector entry
// ((row * NR + k) * DIM + c). The element record, the local row indices and the block's row tables are fetched from HBM once
// per block for all NR vectors (later sub-batches find them in L2); the LDS holds NRS vectors at a time.
// Gating: with ctl != null the kernel belongs to PCG iteration it = itLocal + ctl[0]; it is a no-op once every right-hand side
// has converged (rr_k(it) <= ctl[2 + k]) and accumulates delta_k = (w_k, u_k) into scal[((it + 1) NR + k) 4 + 1].
// blockList (may be null = all) selects the element blocks / row chunks of this launch: the distributed solver runs the
// blocks without halo columns while the halo exchange is in flight and the others after it.
// ------------------------------------------------------------------------------------------------
template <int NR> DEV bool cg_all_done(const double *scal, const double *ctl, int it) {
    bool all = true;
#pragma unroll
    for (int k = 0; k < NR; ++k) all = all && (scal[((int64_t)it * NR + k) * 4 + 2] <= ctl[2 + k]);
    return all;
}

template <int DIM, int DEG, int MAT, int NR, int NRS>
__global__ void __launch_bounds__(MF_BLOCK) k_mf_cluster_nr(SpmvMfArgs a, const double *__restrict__ x, double *__restrict__ y, double *dotOut,
                                                            double *scal, int it, const double *ctl, const int32_t *__restrict__ blockList,
                                                            int64_t nList) {
    constexpr int NPE = (DIM == 3) ? (DEG == 1 ? 4 : 10) : (DEG == 1 ? 3 : 6);
    constexpr int NSB = NR / NRS;
    constexpr int W = NRS * DIM;                                     // doubles per row and sub-batch
    static_assert(NR % NRS == 0, "sub-batch size must divide the batch");
    extern __shared__ __attribute__((aligned(16))) double clacc[];   // accumulators [maxLocal * W] + staged x [maxLocal * W] + dots [8]
    double *xs = clacc + a.clMaxLocal * W;
    double *sdot = xs + a.clMaxLocal * W;
    if (ctl) {
        it += (int)ctl[0];
        if (cg_all_done<NR>(scal, ctl, it)) return;
        dotOut = scal + ((int64_t)(it + 1) * NR) * 4 + 1;
    }
    if (threadIdx.x < 8) sdot[threadIdx.x] = 0.0;
    for (int64_t q = blockIdx.x; q < nList; q += gridDim.x) {
        const int64_t b = blockList ? (int64_t)blockList[q] : q;
        const int u0 = a.clBlockPtr[b], nLocal = a.clBlockPtr[b + 1] - u0;
        const int64_t e0 = a.clElemPtr ? (int64_t)a.clElemPtr[b] : b * a.clBlockElems;
        const int ne = a.clElemPtr ? a.clElemPtr[b + 1] - a.clElemPtr[b] : a.clBlockElems;
        for (int sb = 0; sb < NSB; ++sb) {
            // x of every distinct row of the block, NRS vectors: read once into LDS
            for (int t = threadIdx.x; t < nLocal; t += MF_BLOCK) {
                const int64_t row = a.clEntryRow[u0 + t];
                const double *src = x + (row * NR + sb * NRS) * DIM;
#pragma unroll
                for (int j = 0; j < W; ++j) { xs[t * W + j] = src[j]; clacc[t * W + j] = 0.0; }
            }
            __syncthreads();
            // (a block may hold more elements than lanes: rounds of MF_BLOCK, see k_mf_cluster; the element state -- LDS offsets of its nodes'
            // rows, gradients, volume -- is shared by the NRS vectors of the sub-batch and fetched again per sub-batch and round)
            for (int base = 0; base < ne; base += MF_BLOCK) {
            const int64_t e = e0 + base + threadIdx.x;
            const bool active = base + (int)threadIdx.x < ne && e < a.nElem;
            if (active) {
                int li[NPE];
                double gl[DIM + 1][DIM];
                const double *g = a.geo + (a.clElemPerm ? (int64_t)a.clElemPerm[e] : e) * a.geoStride;   // record of the original element
#pragma unroll
                for (int j = 0; j < NPE; ++j) li[j] = (int)a.clLocalIdx[e * NPE + j] * W;
#pragma unroll
                for (int k = 0; k <= DIM; ++k)
#pragma unroll
                    for (int d = 0; d < DIM; ++d) gl[k][d] = g[k * DIM + d];
                const double vol = g[12];
#pragma unroll 1
                for (int kk = 0; kk < NRS; ++kk) {
                    const double *xk = xs + kk * DIM;
                    double *ak = clacc + kk * DIM;
                    double xl[NPE][DIM];
#pragma unroll
                    for (int j = 0; j < NPE; ++j)
#pragma unroll
                        for (int d = 0; d < DIM; ++d) xl[j][d] = xk[li[j] + d];
                    elem_forces_bilinear<DIM, DEG, MAT>(g, vol, gl, gl, xl, [&](int j, const double *fv) {
#pragma unroll
                        for (int d = 0; d < DIM; ++d) unsafeAtomicAdd(&ak[li[j] + d], fv[d]);
                    });
                }
            }
            }
            __syncthreads();
            double dl[NRS];
#pragma unroll
            for (int kk = 0; kk < NRS; ++kk) dl[kk] = 0.0;
            for (int t = threadIdx.x; t < nLocal; t += MF_BLOCK) {
                const int dest = a.clEntryDest[u0 + t];
                if (dest == -2) continue;                                  // row owned by another rank
                if (dest >= 0) {
                    double *o = a.clIfaceBuf + ((int64_t)dest * NR + sb * NRS) * DIM;
#pragma unroll
                    for (int j = 0; j < W; ++j) o[j] = clacc[t * W + j];
                    continue;
                }
                const int64_t row = a.clEntryRow[u0 + t];
#pragma unroll
                for (int kk = 0; kk < NRS; ++kk)
#pragma unroll
                    for (int d = 0; d < DIM; ++d) {
                        const int64_t gi = (row * NR + sb * NRS + kk) * DIM + d;
                        double v = clacc[t * W + kk * DIM + d];
                        if (a.fixedMask && a.fixedMask[row * DIM + d]) v = 0.0;
                        y[gi] = v;
                        if (dotOut) dl[kk] += v * x[gi];
                    }
            }
            if (dotOut) {
#pragma unroll
                for (int kk = 0; kk < NRS; ++kk) {
                    const double v = wave_sum(dl[kk]);
                    if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(&sdot[sb * NRS + kk], v);
                }
            }
            __syncthreads();
        }
    }
    if (dotOut) {
        __syncthreads();
        if (threadIdx.x < NR) unsafeAtomicAdd(&dotOut[threadIdx.x * 4], sdot[threadIdx.x]);
    }
}

// second pass of the cluster operator for NR interleaved vectors: y_row = sum of the row's interface partials (streamed in
// row order), in the compact numbering of the interface rows
template <int DIM, int NR, int NRS>
__global__ void __launch_bounds__(256) k_mf_rows_nr(SpmvMfArgs a, const double *__restrict__ fbuf, const double *__restrict__ x,
                                                    double *__restrict__ y, double *dotOut, double *scal, int it, const double *ctl) {
    constexpr int NSB = NR / NRS;
    constexpr int W = NRS * DIM;
    extern __shared__ __attribute__((aligned(16))) double mfacc[];   // [maxRows * W] + dots [8]
    double *sdot = mfacc + a.maxRows * W;
    if (ctl) {
        it += (int)ctl[0];
        if (cg_all_done<NR>(scal, ctl, it)) return;
        dotOut = scal + ((int64_t)(it + 1) * NR) * 4 + 1;
    }
    if (threadIdx.x < 8) sdot[threadIdx.x] = 0.0;
    for (int64_t chunk = blockIdx.x; chunk < a.nChunk; chunk += gridDim.x) {
        const int r0 = a.chunkRow[chunk], r1 = a.chunkRow[chunk + 1];
        const int nr = r1 - r0;
        const int64_t kb = a.pairPtr[chunk], ke = a.pairPtr[chunk + 1];
        for (int sb = 0; sb < NSB; ++sb) {
            for (int t = threadIdx.x; t < nr * W; t += 256) mfacc[t] = 0.0;
            __syncthreads();
            for (int64_t k = kb + threadIdx.x; k < ke; k += 256) {
                const int lr = a.pairRow[k];
                const double *src = fbuf + (k * NR + sb * NRS) * DIM;
                double v[W];
#pragma unroll
                for (int j = 0; j < W; ++j) v[j] = src[j];
#pragma unroll
                for (int j = 0; j < W; ++j) unsafeAtomicAdd(&mfacc[lr * W + j], v[j]);
            }
            __syncthreads();
            double dl[NRS];
#pragma unroll
            for (int kk = 0; kk < NRS; ++kk) dl[kk] = 0.0;
            for (int t = threadIdx.x; t < nr; t += 256) {
                const int64_t row = a.rowMap[r0 + t];
#pragma unroll
                for (int kk = 0; kk < NRS; ++kk)
#pragma unroll
                    for (int d = 0; d < DIM; ++d) {
                        const int64_t gi = (row * NR + sb * NRS + kk) * DIM + d;
                        double v = mfacc[t * W + kk * DIM + d];
                        if (a.fixedMask && a.fixedMask[row * DIM + d]) v = 0.0;
                        y[gi] = v;
                        if (dotOut) dl[kk] += v * x[gi];
                    }
            }
            if (dotOut) {
#pragma unroll
                for (int kk = 0; kk < NRS; ++kk) {
                    const double v = wave_sum(dl[kk]);
                    if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(&sdot[sb * NRS + kk], v);
                }
            }
            __syncthreads();
        }
    }
    if (dotOut) {
        __syncthreads();
        if (threadIdx.x < NR) unsafeAtomicAdd(&dotOut[threadIdx.x * 4], sdot[threadIdx.x]);
    }
}

// assembled block-CSR SpMV for NR interleaved vectors (the operator of linear elements, scalar operators and
// caller-supplied matrices); NRS vectors per pass through the LDS partials
template <int DIM, int NR, int NRS>
__global__ void __launch_bounds__(256) k_spmv_nr(SpmvArgs a, const double *__restrict__ x, double *__restrict__ y, double *dotOut,
                                                 double *scal, int it, const double *ctl, const int32_t *__restrict__ chunkList, int64_t nList) {
    constexpr int NB = DIM * DIM;
    constexpr int NSB = NR / NRS;
    extern __shared__ __attribute__((aligned(16))) double part[];  // [NRS * DIM][chunkSlots] + dots [8]
    const int CS = a.chunkSlots;
    double *sdot = part + NRS * DIM * CS;
    if (ctl) {
        it += (int)ctl[0];
        if (cg_all_done<NR>(scal, ctl, it)) return;
        dotOut = scal + ((int64_t)(it + 1) * NR) * 4 + 1;
    }
    if (threadIdx.x < 8) sdot[threadIdx.x] = 0.0;
    for (int64_t q = blockIdx.x; q < nList; q += gridDim.x) {
        const int64_t chunk = chunkList ? (int64_t)chunkList[q] : q;
        const int r0 = a.chunkRow[chunk], r1 = a.chunkRow[chunk + 1];
        const int s0 = a.rowPtr[r0];
        const int ns = a.rowPtr[r1] - s0;
        for (int sb = 0; sb < NSB; ++sb) {
            for (int t = threadIdx.x; t < ns; t += 256) {
                const int64_t s = (int64_t)s0 + t;
                const int64_t col = a.colIdx[s];
                double A[NB];
                if (a.vals32) {          // (uniform over the launch: the FP32 copy of the matrix a multigrid level keeps for its smoother)
#pragma unroll
                    for (int c = 0; c < NB; ++c) A[c] = (double)a.vals32[tiled_index(s, c, NB)];
                } else {
#pragma unroll
                    for (int c = 0; c < NB; ++c) A[c] = a.vals[tiled_index(s, c, NB)];
                }
#pragma unroll
                for (int kk = 0; kk < NRS; ++kk) {
                    double xv[DIM];
#pragma unroll
                    for (int d = 0; d < DIM; ++d) xv[d] = x[(col * NR + sb * NRS + kk) * DIM + d];
#pragma unroll
                    for (int c = 0; c < DIM; ++c) {
                        double v = 0;
#pragma unroll
                        for (int d = 0; d < DIM; ++d) v += A[c * DIM + d] * xv[d];
                        part[(kk * DIM + c) * CS + t] = v;
                    }
                }
            }
            __syncthreads();
            const int nscalar = (r1 - r0) * NRS * DIM;
            double dl[NRS];
#pragma unroll
            for (int kk = 0; kk < NRS; ++kk) dl[kk] = 0.0;
            for (int idx = threadIdx.x; idx < nscalar; idx += 256) {
                const int rl = idx / (NRS * DIM), kc = idx - rl * (NRS * DIM);
                const int kk = kc / DIM, c = kc - kk * DIM;
                const int64_t r = r0 + rl;
                const int b = a.rowPtr[r] - s0, e = a.rowPtr[r + 1] - s0;
                double v = 0;
                for (int t = b; t < e; ++t) v += part[kc * CS + t];
                if (a.fixedMask && a.fixedMask[r * DIM + c]) v = 0.0;
                const int64_t gi = (r * NR + sb * NRS + kk) * DIM + c;
                y[gi] = v;
                if (dotOut) {
                    const double pr = v * x[gi];
#pragma unroll
                    for (int k2 = 0; k2 < NRS; ++k2) dl[k2] += (k2 == kk) ? pr : 0.0;
                }
            }
            if (dotOut) {
#pragma unroll
                for (int kk = 0; kk < NRS; ++kk) {
                    const double v = wave_sum(dl[kk]);
                    if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(&sdot[sb * NRS + kk], v);
                }
            }
            __syncthreads();
        }
    }
    if (dotOut) {
        __syncthreads();
        if (threadIdx.x < NR) unsafeAtomicAdd(&dotOut[threadIdx.x * 4], sdot[threadIdx.x]);
    }
}

// flags the element blocks (cluster operator) / row chunks (assembled SpMV) that read a halo column
__global__ void __launch_bounds__(256) k_flag_halo_blocks(int64_t nBlocks, const int32_t *__restrict__ blockPtr, const int32_t *__restrict__ entryDest,
                                                          uint8_t *__restrict__ flag) {
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < nBlocks; b += (int64_t)gridDim.x * 256) {
        bool halo = false;
        for (int u = blockPtr[b]; u < blockPtr[b + 1]; ++u) halo |= entryDest[u] == -2;
        flag[b] = halo;
    }
}
__global__ void __launch_bounds__(256) k_flag_halo_chunks(int64_t nChunk, const int32_t *__restrict__ chunkRow, const int32_t *__restrict__ rowPtr,
                                                          const int32_t *__restrict__ colIdx, int64_t nOwnedCols, uint8_t *__restrict__ flag) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < nChunk; c += (int64_t)gridDim.x * 256) {
        bool halo = false;
        for (int s = rowPtr[chunkRow[c]]; s < rowPtr[chunkRow[c + 1]]; ++s) halo |= colIdx[s] >= nOwnedCols;
        flag[c] = halo;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers (the instantiation tables: mfh_dispatch.hh)
// ------------------------------------------------------------------------------------------------

void launch_geometry(int dim, int /*deg*/, int /*mat*/, int64_t nElem, const int32_t *elemNodes, int npe, const double *vertPos,
                     const double *matParams, int matMode, double *geo, int geoStride, int *negCount, hipStream_t s) {
    const int grid = (int)((nElem + 255) / 256);
    const size_t lds = (size_t)256 * (geoStride + 1) * sizeof(double);
    with_dim(dim, [&](auto D) { launch_k(k_geometry<D()>, dim3(grid), dim3(256), lds, s, nElem, elemNodes, npe, vertPos, matParams, matMode, geo, geoStride, negCount); });
    CHECK_LAUNCH();
}

void launch_assemble_gather(const AsmArgs &a, hipStream_t s) {
    if (a.nChunk == 0) return;
    if (a.mat == MAT_GEOM && !a.sigma) throw Error(MFH_ERR_STATE, "geometric-stiffness assembly without a prestress field");
    if (a.mat == MAT_MASS_RHO && !a.density) throw Error(MFH_ERR_STATE, "density-weighted mass assembly without a density field");
    size_t lds = (size_t)(mat_is_scalar(a.mat) ? 1 : a.dim * a.dim) * (a.chunkSlots + 2) * sizeof(double);
    if (a.deg == 2 && a.mat != MAT_MASS && a.mat != MAT_MASS_RHO) lds += (size_t)a.npe * a.npe * (4 * sizeof(double) + sizeof(uint32_t));   // pair table
    // (the token of the deterministic flavour sits behind the pair-table region whether or not the flavour has a table)
    if (a.det) lds = (size_t)(mat_is_scalar(a.mat) ? 1 : a.dim * a.dim) * (a.chunkSlots + 2) * sizeof(double) + (size_t)a.npe * a.npe * (4 * sizeof(double) + sizeof(uint32_t)) + 16;
    // the density-weighted mass (ensure_mass with a density field set) and the geometric stiffness (H : sigma_e, ensure_geometric) exist for the
    // gather assembly only: the atomic variant and the dense element matrices never see them.
    // The deterministic flavour is an instantiation of its own (barriers inside the contribution loop): the default kernels keep the plain loop
    with_elem_asm<MAT_MASS_RHO, MAT_GEOM>(a, [&](auto D, auto G, auto M) {
        with_bool(a.upperOnly, [&](auto UP) { with_bool(a.det, [&](auto DT) {
            launch_k(k_assemble_gather<D(), G(), M(), UP(), DT()>, dim3((unsigned)a.nChunk), dim3(256), lds, s, a);
        }); });
    });
    CHECK_LAUNCH();
}

void launch_chunk_keys(const AsmArgs &a, uint32_t *keys, hipStream_t s) {
    if (a.nChunk == 0) return;
    hipLaunchKernelGGL(k_chunk_keys, dim3((unsigned)((a.nChunk + 255) / 256)), dim3(256), 0, s, a.nChunk, a.contribPtr, a.contribCode,
                       a.chunkElemBase, (uint32_t)(a.npe * a.npe), keys);
    CHECK_LAUNCH();
}

bool launch_pack_codes(int64_t nChunk, const int64_t *contribPtr, uint32_t *contribCode, int npe, int32_t *chunkElemBase, int *flag, hipStream_t s) {
    if (nChunk == 0) return true;
    MFH_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_pack_codes, dim3((unsigned)nChunk), dim3(64), 0, s, nChunk, contribPtr, contribCode, (uint32_t)(npe * npe), chunkElemBase, flag, 0);
    CHECK_LAUNCH();
    int h = 0;
    MFH_HIP(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, s));
    MFH_HIP(hipStreamSynchronize(s));
    if (h) return false;      // some chunk gathers from elements more than 2^25 apart: the codes stay absolute
    hipLaunchKernelGGL(k_pack_codes, dim3((unsigned)nChunk), dim3(64), 0, s, nChunk, contribPtr, contribCode, (uint32_t)(npe * npe), chunkElemBase, flag, 1);
    CHECK_LAUNCH();
    return true;
}

void launch_assemble_atomic(const AsmArgs &a, hipStream_t s) {
    const int64_t total = a.nElem * a.npe * a.npe;
    const int grid = grid_for(total, 256 * 32);
    with_elem_asm(a, [&](auto D, auto G, auto M) { launch_k(k_assemble_atomic<D(), G(), M()>, dim3(grid), dim3(256), 0, s, a); });
    CHECK_LAUNCH();
}

void launch_element_stiffness(const AsmArgs &a, int64_t first, int64_t count, double *KeOut, hipStream_t s) {
    const int grid = grid_for(count * a.npe * a.npe);
    with_elem_asm(a, [&](auto D, auto G, auto M) { launch_k(k_element_stiffness<D(), G(), M()>, dim3(grid), dim3(256), 0, s, a, first, count, KeOut); });
    CHECK_LAUNCH();
}

void launch_elem_abs_rowsums(const AsmArgs &a, double *out, int gridCap, hipStream_t s) {
    if (a.nElem <= 0) return;
    const int grid = grid_for(a.nElem * a.npe, std::max(1, std::min(gridCap, 8192)));
    with_elem(a, [&](auto D, auto G, auto M) { launch_k(k_elem_abs_rowsums<D(), G(), M()>, dim3(grid), dim3(256), 0, s, a, out); });
    CHECK_LAUNCH();
}

static LoadArgs make_load_args(const AsmArgs &a, const int32_t *elemNodes, const int32_t *dofForNode, const double *intGrad,
                               const double *cstrain) {
    LoadArgs l{};
    l.nElem = a.nElem; l.npe = a.npe; l.geoStride = a.geoStride; l.geo = a.geo; l.elemNodes = elemNodes; l.dofForNode = dofForNode;
    for (int k = 0; k < 2 * a.npe; ++k) l.intGrad[k] = intGrad[k];
    for (int k = 0; k < 6; ++k) l.cstrain[k] = cstrain ? cstrain[k] : 0.0;
    return l;
}

void launch_constant_strain_load(const AsmArgs &a, const int32_t *elemNodes, const int32_t *dofForNode, const double *intGrad,
                                 const double *cstrain, const double *deltaP, double *out, hipStream_t s) {
    const LoadArgs l = make_load_args(a, elemNodes, dofForNode, intGrad, cstrain);
    const int grid = grid_for(a.nElem * a.npe, 8192);
    with_elem(a, [&](auto D, auto G, auto M) { launch_k(k_constant_strain_load<D(), G(), M()>, dim3(grid), dim3(256), 0, s, l, deltaP, out); });
    CHECK_LAUNCH();
}

void launch_edge_covariance(int64_t nElem, int dim, int npe, const int32_t *elemNodes, const double *vertPos, double *out6, hipStream_t s) {
    if (nElem <= 0) return;
    hipLaunchKernelGGL(k_edge_covariance, dim3(grid_for(nElem)), dim3(256), 0, s, nElem, dim, npe, elemNodes, vertPos, out6);
    CHECK_LAUNCH();
}
void launch_neumann_load(int64_t nBE, int npbe, int dim, const double *w6, const int32_t *bdryElemNodes, const int32_t *dofForNode, const double *bdryVol,
                         const double *traction, double *out, hipStream_t s) {
    if (nBE <= 0) return;
    NeumannArgs a{nBE, npbe, dim, {w6[0], w6[1], w6[2], w6[3], w6[4], w6[5]}};
    hipLaunchKernelGGL(k_neumann_load, dim3(grid_for(nBE * npbe)), dim3(256), 0, s, a, bdryElemNodes, dofForNode, bdryVol, traction, out);
    CHECK_LAUNCH();
}
void launch_average_strain(const AsmArgs &a, const int32_t *elemNodes, const double *intGrad, const double *uNodes, double *out,
                           int wantStress, const double *uFixed, const double *deltaP, hipStream_t s, const double *addStrain, double *integral) {
    const LoadArgs l = make_load_args(a, elemNodes, nullptr, intGrad, nullptr);
    const int grid = grid_for(a.nElem, integral ? 1024 : 8192);
    StrainShift add{};
    if (addStrain) { add.on = 1; for (int q = 0; q < a.dim * (a.dim + 1) / 2; ++q) add.v[q] = addStrain[q]; }
    with_elem(a, [&](auto D, auto G, auto M) {
        launch_k(k_average_strain<D(), G(), M()>, dim3(grid), dim3(256), 0, s, l, uNodes, out, wantStress, uFixed, deltaP, add, integral);
    });
    CHECK_LAUNCH();
}

void launch_apply_delta_K(const AsmArgs &a, const int32_t *elemNodes, const int32_t *dofForNode, const double *intGrad,
                          const double *uNodes, const double *deltaP, double *out, hipStream_t s) {
    const LoadArgs l = make_load_args(a, elemNodes, dofForNode, intGrad, nullptr);
    const int grid = grid_for(a.nElem, 8192);
    with_elem(a, [&](auto D, auto G, auto M) { launch_k(k_apply_delta_K<D(), G(), M()>, dim3(grid), dim3(256), 0, s, l, uNodes, deltaP, out); });
    CHECK_LAUNCH();
}

void launch_mutual_energies(const AsmArgs &a, const int32_t *elemNodes, const double *intGrad, const double *w, int64_t nNode,
                            const double *deltaP, double *out, hipStream_t s) {
    const LoadArgs l = make_load_args(a, elemNodes, nullptr, intGrad, nullptr);
    const int fl = a.dim * (a.dim + 1) / 2;
    const dim3 grid(grid_for(a.nElem, 4096), fl * (fl + 1) / 2);
    with_elem(a, [&](auto D, auto G, auto M) { launch_k(k_mutual_energies<D(), G(), M()>, grid, dim3(256), 0, s, l, w, nNode, deltaP, out); });
    CHECK_LAUNCH();
}

void launch_strain_field(const AsmArgs &a, const int32_t *elemNodes, const double *intGrad, const double *uNodes, int wantStress,
                         double *out, hipStream_t s) {
    const LoadArgs l = make_load_args(a, elemNodes, nullptr, intGrad, nullptr);
    const int grid = grid_for(a.nElem, 8192);
    with_elem(a, [&](auto D, auto G, auto M) { launch_k(k_strain_field<D(), G(), M()>, dim3(grid), dim3(256), 0, s, l, uNodes, wantStress, out); });
    CHECK_LAUNCH();
}

void launch_sym_measures(int dim, int64_t n, const double *field, int what, double *vm, double *eval, double *evec, hipStream_t s) {
    if (n <= 0) return;
    const int grid = grid_for(n, 8192);
    with_dim(dim, [&](auto D) { launch_k(k_sym_measures<D()>, dim3(grid), dim3(256), 0, s, n, field, what, vm, eval, evec); });
    CHECK_LAUNCH();
}

void launch_stress_measures(const AsmArgs &a, const int32_t *elemNodes, const double *intGrad, const double *uNodes, int wantStress, int what,
                            double *vm, double *eval, double *evec, hipStream_t s) {
    const LoadArgs l = make_load_args(a, elemNodes, nullptr, intGrad, nullptr);
    const int grid = grid_for(a.nElem, 8192);
    with_elem(a, [&](auto D, auto G, auto M) {
        launch_k(k_stress_measures<D(), G(), M()>, dim3(grid), dim3(256), 0, s, l, uNodes, wantStress, what, vm, eval, evec);
    });
    CHECK_LAUNCH();
}

void launch_peak_von_mises(const AsmArgs &a, const int32_t *elemNodes, const double *intGrad, const double *uNodes, int wantStress,
                           double *partV, int64_t *partI, double *outV, int64_t *outI, hipStream_t s) {
    const LoadArgs l = make_load_args(a, elemNodes, nullptr, intGrad, nullptr);
    const int grid = grid_for(a.nElem, PEAK_GRID_CAP);
    long long *pI = reinterpret_cast<long long *>(partI), *oI = reinterpret_cast<long long *>(outI);
    with_elem(a, [&](auto D, auto G, auto M) { launch_k(k_peak_von_mises<D(), G(), M()>, dim3(grid), dim3(256), 0, s, l, uNodes, wantStress, partV, pI); });
    hipLaunchKernelGGL(k_peak_finish, dim3(1), dim3(256), 0, s, grid, (const double *)partV, (const long long *)pI, outV, oI);
    CHECK_LAUNCH();
}

void launch_peak_of_array(int64_t n, const double *v, double *partV, int64_t *partI, double *outV, int64_t *outI, hipStream_t s) {
    const int grid = grid_for(n, PEAK_GRID_CAP);
    long long *pI = reinterpret_cast<long long *>(partI), *oI = reinterpret_cast<long long *>(outI);
    hipLaunchKernelGGL(k_peak_of_array, dim3(grid), dim3(256), 0, s, n, v, partV, pI);
    hipLaunchKernelGGL(k_peak_finish, dim3(1), dim3(256), 0, s, grid, (const double *)partV, (const long long *)pI, outV, oI);
    CHECK_LAUNCH();
}

void launch_modal_stress_sumsq(const AsmArgs &a, const int32_t *elemNodes, const int32_t *dofForNode, const double *intGrad, const double *U, int64_t ldu, int np,
                               int wantStress, bool first, bool root, double *vm, double *comp, hipStream_t s) {
    if (a.nElem <= 0) return;
    const LoadArgs l = make_load_args(a, elemNodes, dofForNode, intGrad, nullptr);
    const int grid = grid_for(a.nElem, MODAL_STRESS_GRID_CAP);
    with_elem(a, [&](auto D, auto G, auto M) {
        launch_k(k_modal_stress_sumsq<D(), G(), M()>, dim3(grid), dim3(256), 0, s, l, U, ldu, np, wantStress, first ? 1 : 0, root ? 1 : 0, vm, comp);
    });
    CHECK_LAUNCH();
}

void launch_vertex_average(int dim, int npe, int64_t nVert, const int32_t *nodePtr, const int32_t *nodePair, const double *geo, int geoStride,
                           const double *field, int nq, int nComp, double *out, hipStream_t s) {
    if (nVert <= 0) return;
    const int grid = grid_for(nVert);
    for (int c0 = 0; c0 < nComp; c0 += 9) {          // components in register blocks of at most 9 (a full dim x dim tensor in 3D)
        const int cb = std::min(9, nComp - c0);
        with_int<1, 2, 3, 4, 5, 6, 7, 8, 9>(cb, [&](auto CB) {
            launch_k(k_vertex_average<CB()>, dim3(grid), dim3(256), 0, s, nVert, nodePtr, nodePair, npe, dim + 1, geo, geoStride, field, nq, nComp, c0, out);
        });
    }
    CHECK_LAUNCH();
}

void launch_boundary_strain_field(const AsmArgs &a, const int32_t *elemNodes, const double *intGrad, int64_t nBE,
                                  const int32_t *bdryParent, const int32_t *bdryElemNodes, int npbe, const double *uNodes,
                                  int wantStress, double *out, hipStream_t s) {
    if (nBE == 0) return;
    const LoadArgs l = make_load_args(a, elemNodes, nullptr, intGrad, nullptr);
    const int grid = grid_for(nBE, 8192);
    with_elem(a, [&](auto D, auto G, auto M) {
        launch_k(k_boundary_strain_field<D(), G(), M()>, dim3(grid), dim3(256), 0, s, l, nBE, bdryParent, bdryElemNodes, npbe, uNodes, wantStress, out);
    });
    CHECK_LAUNCH();
}

void launch_mutual_energy_differential(const AsmArgs &a, const int32_t *elemNodes, const double *intGrad, const double *w,
                                       int64_t nNode, int64_t nVert, double *out, hipStream_t s) {
    const LoadArgs l = make_load_args(a, elemNodes, nullptr, intGrad, nullptr);
    const int fl = a.dim * (a.dim + 1) / 2;
    const dim3 grid(grid_for(a.nElem, 4096), fl * (fl + 1) / 2);
    with_elem(a, [&](auto D, auto G, auto M) { launch_k(k_mutual_energy_differential<D(), G(), M()>, grid, dim3(256), 0, s, l, w, nNode, nVert, out); });
    CHECK_LAUNCH();
}

void launch_average_gradient(const AsmArgs &a, const int32_t *elemNodes, const double *intGrad, const double *uNodes, double *out,
                             hipStream_t s) {
    const LoadArgs l = make_load_args(a, elemNodes, nullptr, intGrad, nullptr);
    const int grid = grid_for(a.nElem, 8192);
    with_dim_deg(a.dim, a.deg, [&](auto D, auto G) { launch_k(k_average_gradient<D(), G()>, dim3(grid), dim3(256), 0, s, l, uNodes, out); });
    CHECK_LAUNCH();
}

// persistent workgroups; a multiple of 8 (xcd_span)
static int persistent_grid(int64_t nItems, int cap) { return (int)std::max<int64_t>(8, std::min<int64_t>(cap, (nItems + 7) / 8 * 8)); }
static int spmv_grid(const SpmvArgs &a) { return persistent_grid(a.nChunk, 256 * 8); }

// mode: 0 plain (dotOut optional), 1 classic PCG bookkeeping, 2 Chronopoulos-Gear bookkeeping (one right-hand side);
// chunkList / nList: the chunks of this launch (null = all)
static void launch_spmv_mode(const SpmvArgs &a_, int mode, const double *x, double *y, double *dotOut, double *scal, int it, const double *stopPtr,
                             const int32_t *chunkList, int64_t nList, hipStream_t s) {
    const int64_t n = chunkList ? nList : a_.nChunk;
    if (n <= 0) return;
    SpmvArgs ad = a_;
    ad.det = t_det;
    const SpmvArgs &a = ad;
    const size_t lds = ((size_t)a.dim * a.chunkSlots + 16) * sizeof(double);
    const int grid = det_grid(persistent_grid(n, 256 * 8));
    if (a.kron) {           // one value per block (MFH_OP_MASS_VECTOR): plain product or the classic PCG's bookkeeping
        if (mode == 2 || a.vals32 || (a.dim != 2 && a.dim != 3)) throw mfh::Error(MFH_ERR_UNSUPPORTED, "k_spmv_kron serves the plain product and the classic PCG loop in 2D / 3D only");
        with_dim(a.dim, [&](auto D) { with_int<1, 0>(mode, [&](auto MODE) {
            launch_k(k_spmv_kron<D(), MODE()>, dim3(grid), dim3(256), lds, s, a, x, y, dotOut, scal, it, stopPtr, chunkList, nList);
        }); });
    } else {
        with_dim132(a.dim, [&](auto D) { with_int<0, 1, 2>(mode, [&](auto MODE) {
            launch_k(k_spmv<D(), MODE()>, dim3(grid), dim3(256), lds, s, a, x, y, dotOut, scal, it, stopPtr, chunkList, nList);
        }); });
    }
    if (dotOut || scal) launch_det_finish(s);
    CHECK_LAUNCH();
}

void launch_spmv(const SpmvArgs &a, const double *x, double *y, double *dotOut, hipStream_t s) {
    launch_spmv_mode(a, 0, x, y, dotOut, nullptr, 0, nullptr, nullptr, 0, s);
}

void launch_row_sums(int64_t nRows, const int32_t *rowPtr, const int32_t *colIdx, const double *vals, int rep, bool upperOnly, double *out, hipStream_t s) {
    if (nRows <= 0) return;
    const int grid = grid_for(nRows, 8192);
    with_bool(upperOnly, [&](auto UP) { launch_k(k_row_sums<UP()>, dim3(grid), dim3(256), 0, s, nRows, rowPtr, colIdx, vals, rep, out); });
    CHECK_LAUNCH();
}

void launch_divergence(int dim, int64_t nNode, const int32_t *nodePtr, const int32_t *nodePair, const double *geo, int geoStride, const double *elemVec,
                       double *out, hipStream_t s) {
    if (nNode <= 0) return;
    const int grid = grid_for(nNode, 8192);
    with_dim(dim, [&](auto D) { launch_k(k_divergence<D()>, dim3(grid), dim3(256), 0, s, nNode, nodePtr, nodePair, geo, geoStride, elemVec, out); });
    CHECK_LAUNCH();
}

// y = K x from the upper-triangle storage (k_spmv_sym); nRows = rows of y (zeroed here); dotOut (optional): *dotOut += x . y
void launch_spmv_sym(const SpmvArgs &a, int64_t nRows, const double *x, double *y, double *dotOut, hipStream_t s) {
    if (a.nChunk <= 0) return;
    if (a.kron) throw Error(MFH_ERR_UNSUPPORTED, "k_spmv_sym reads dense blocks; the one-value-per-block storage (MFH_OP_MASS_VECTOR) has k_spmv_kron only");
    MFH_HIP(hipMemsetAsync(y, 0, (size_t)nRows * a.dim * sizeof(double), s));
    const size_t lds = ((size_t)a.dim * a.chunkSlots + 16) * sizeof(double) + (size_t)a.chunkSlots * sizeof(unsigned short);
    const int grid = spmv_grid(a);
    with_dim132(a.dim, [&](auto D) { launch_k(k_spmv_sym<D()>, dim3(grid), dim3(256), lds, s, a, nRows, x, y); });
    CHECK_LAUNCH();
    if (dotOut) launch_dot(nRows * a.dim, x, y, dotOut, s);
}

void launch_pcg_spmv(const SpmvArgs &a, const double *p, double *Ap, double *scal, int it, const double *stopPtr, hipStream_t s) {
    launch_spmv_mode(a, 1, p, Ap, nullptr, scal, it, stopPtr, nullptr, 0, s);
}

void launch_spmv_mf(const SpmvMfArgs &a, const double *x, double *y, double *dotOut, double *scal, int it, const double *stopPtr,
                    bool pcg, hipStream_t s) {
    if (a.nChunk == 0) return;
    const int bs = mat_is_scalar(a.mat) ? 1 : a.dim;
    const size_t lds = ((size_t)a.maxRows * bs + 16) * sizeof(double);
    const int grid = persistent_grid(a.nChunk, 256 * 8);
    with_elem_asm(a, [&](auto D, auto G, auto M) {
        if (pcg) launch_k(k_spmv_mf<D(), G(), M(), true>, dim3(grid), dim3(256), lds, s, a, x, y, (double *)nullptr, scal, it, stopPtr);
        else launch_k(k_spmv_mf<D(), G(), M(), false>, dim3(grid), dim3(256), lds, s, a, x, y, dotOut, (double *)nullptr, 0, (const double *)nullptr);
    });
    CHECK_LAUNCH();
}

static void launch_mf_rows_mode(const SpmvMfArgs &a_, int mode, const double *x, double *y, double *dotOut, double *scal, int it, const double *stopPtr,
                                hipStream_t s) {
    if (a_.nChunk == 0) return;
    SpmvMfArgs ad = a_;
    ad.det = t_det;
    const SpmvMfArgs &a = ad;
    const size_t lds = ((size_t)a.maxRows * a.dim + 16) * sizeof(double);
    const int grid = det_grid(persistent_grid(a.nChunk, 256 * 8));
    with_dim(a.dim, [&](auto D) { with_int<0, 1, 2>(mode, [&](auto MODE) { with_bool(a.det.partials != nullptr, [&](auto DT) {
        launch_k(k_mf_rows<D(), MODE(), DT()>, dim3(grid), dim3(256), lds, s, a, (const double *)a.sig, x, y, dotOut, scal, it, stopPtr);
    }); }); });
    if (dotOut || scal) launch_det_finish(s);
    CHECK_LAUNCH();
}

// two-pass matrix-free elasticity operator (k_mf_stress + k_mf_rows)
void launch_spmv_mf2(const SpmvMfArgs &a, const double *x, double *y, double *dotOut, double *scal, int it, const double *stopPtr,
                     bool pcg, hipStream_t s) {
    if (a.nChunk == 0) return;
    const int gridE = persistent_grid((a.nElem + 255) / 256, 256 * 32);   // persistent over element groups
    with_elem(a, [&](auto D, auto G, auto M) {
        launch_k(k_mf_forces<D(), G(), M()>, dim3(gridE), dim3(256), 0, s, a, x, a.sig, pcg ? (const double *)scal : (const double *)nullptr, it, stopPtr);
    });
    CHECK_LAUNCH();
    launch_mf_rows_mode(a, pcg ? 1 : 0, x, y, pcg ? nullptr : dotOut, pcg ? scal : nullptr, pcg ? it : 0, pcg ? stopPtr : nullptr, s);
}

// cluster variant of the matrix-free elasticity operator: k_mf_cluster over the blocks of blockList (null = all) ...
static void launch_mf_cluster_mode(const SpmvMfArgs &a_, int mode, const double *x, double *y, double *dotOut, double *scal, int it,
                                   const double *stopPtr, const int32_t *blockList, int64_t nList, hipStream_t s) {
    if (nList <= 0) return;
    SpmvMfArgs ad = a_;
    ad.det = t_det;
    const SpmvMfArgs &a = ad;
    const size_t ldsC = ((size_t)(a.det.partials ? 5 : 2) * a.clMaxLocal * a.dim + 16) * sizeof(double);
    const int gridC = det_grid((int)std::min<int64_t>(nList, 256 * 64));
    // the deterministic flavour (per-wave accumulators) is an instantiation of its own
    with_elem(a, [&](auto D, auto G, auto M) { with_int<0, 1, 2>(mode, [&](auto MODE) {
        with_bool(a.vertPos != nullptr, [&](auto GV) { with_bool(a.det.partials != nullptr, [&](auto DT) {
            launch_k(k_mf_cluster<D(), G(), M(), MODE(), GV(), DT()>, dim3(gridC), dim3(MF_BLOCK), ldsC, s, a, x, y, dotOut, scal, it, stopPtr, blockList, nList);
        }); });
    }); });
    if (dotOut || scal) launch_det_finish(s);
    CHECK_LAUNCH();
}

// constantStrainLoad through the cluster operator (see mfh_internal.hh): the SHIFT flavour of k_mf_cluster over all blocks, then the interface pass
void launch_mf_cluster_constant_strain(const SpmvMfArgs &a_, const double *cstrainFlat, double *y, hipStream_t s) {
    SpmvMfArgs ad = a_;
    ad.det = DetBuf{};
    ad.fixedMask = nullptr;
    for (int q = 0; q < 6; ++q) ad.shift[q] = q < ad.dim * (ad.dim + 1) / 2 ? cstrainFlat[q] : 0.0;
    const SpmvMfArgs &a = ad;
    if (a.clBlocks > 0) {
        const size_t ldsC = ((size_t)2 * a.clMaxLocal * a.dim + 16) * sizeof(double);
        const int gridC = (int)std::min<int64_t>(a.clBlocks, 256 * 64);
        with_elem(a, [&](auto D, auto G, auto M) { with_bool(a.vertPos != nullptr, [&](auto GV) {
            launch_k(k_mf_cluster<D(), G(), M(), 0, GV(), false, true>, dim3(gridC), dim3(MF_BLOCK), ldsC, s, a, (const double *)y, y, (double *)nullptr, (double *)nullptr, 0,
                     (const double *)nullptr, (const int32_t *)nullptr, a.clBlocks);
        }); });
        CHECK_LAUNCH();
    }
    launch_mf_rows_mode(a, 0, y, y, nullptr, nullptr, 0, nullptr, s);
}

// ... followed by k_mf_rows over the interface partials
void launch_spmv_mf_cluster(const SpmvMfArgs &a, const double *x, double *y, double *dotOut, double *scal, int it, const double *stopPtr,
                            bool pcg, hipStream_t s) {
    const int mode = pcg ? 1 : 0;
    launch_mf_cluster_mode(a, mode, x, y, pcg ? nullptr : dotOut, pcg ? scal : nullptr, pcg ? it : 0, pcg ? stopPtr : nullptr, nullptr, a.clBlocks, s);
    launch_mf_rows_mode(a, mode, x, y, pcg ? nullptr : dotOut, pcg ? scal : nullptr, pcg ? it : 0, pcg ? stopPtr : nullptr, s);
}

// ---- operators of the batched / distributed PCG (the batch shapes: select_batch / select_batch_1d, mfh_dispatch.hh)
bool op_batch_supported(int dim, int nr) { return nr == 1 || select_batch_1d(dim, nr, [](auto, auto, auto) {}); }

void launch_mf_cluster_nr(const SpmvMfArgs &a, int NR, const double *x, double *y, double *dotOut, double *scal, int it, const double *ctl,
                          const int32_t *blockList, int64_t nList, hipStream_t s) {
    if (nList <= 0) return;
    if (NR == 1) { launch_mf_cluster_mode(a, a.pcgMode ? a.pcgMode : (ctl ? 2 : 0), x, y, dotOut, scal, it, ctl, blockList, nList, s); return; }
    // only the instantiated batch sizes: any other NR would run a kernel built for a different vector stride
    if (!op_batch_supported(a.dim, NR)) throw Error(MFH_ERR_UNSUPPORTED, "cluster operator: unsupported batch size " + std::to_string(NR));
    const int gridC = (int)std::min<int64_t>(nList, 256 * 64);
    with_batch(a.dim, NR, "cluster operator: unsupported batch size", [&](auto D, auto N, auto NS) { with_int<2, 1>(a.deg, [&](auto G) { with_elasticity(a.mat, [&](auto M) {
        const size_t ldsC = ((size_t)2 * a.clMaxLocal * a.dim * NS() + 8) * sizeof(double);
        launch_k(k_mf_cluster_nr<D(), G(), M(), N(), NS()>, dim3(gridC), dim3(MF_BLOCK), ldsC, s, a, x, y, dotOut, scal, it, ctl, blockList, nList);
    }); }); });
    CHECK_LAUNCH();
}

void launch_mf_rows_nr(const SpmvMfArgs &a, int NR, const double *x, double *y, double *dotOut, double *scal, int it, const double *ctl, hipStream_t s) {
    if (a.nChunk == 0) return;
    if (NR == 1) { launch_mf_rows_mode(a, a.pcgMode ? a.pcgMode : (ctl ? 2 : 0), x, y, dotOut, scal, it, ctl, s); return; }
    if (!op_batch_supported(a.dim, NR)) throw Error(MFH_ERR_UNSUPPORTED, "cluster operator (interface rows): unsupported batch size " + std::to_string(NR));
    const int grid = persistent_grid(a.nChunk, 256 * 8);
    with_batch(a.dim, NR, "cluster operator (interface rows): unsupported batch size", [&](auto D, auto N, auto NS) {
        const size_t lds = ((size_t)a.maxRows * a.dim * NS() + 8) * sizeof(double);
        launch_k(k_mf_rows_nr<D(), N(), NS()>, dim3(grid), dim3(256), lds, s, a, (const double *)a.sig, x, y, dotOut, scal, it, ctl);
    });
    CHECK_LAUNCH();
}

void launch_spmv_nr(const SpmvArgs &a, int NR, const double *x, double *y, double *dotOut, double *scal, int it, const double *ctl,
                    const int32_t *chunkList, int64_t nList, hipStream_t s) {
    if (nList <= 0) return;
    if (NR == 1) { launch_spmv_mode(a, a.pcgMode ? a.pcgMode : (ctl ? 2 : 0), x, y, dotOut, scal, it, ctl, chunkList, nList, s); return; }
    if (a.kron) throw Error(MFH_ERR_UNSUPPORTED, "assembled SpMV: the batched product reads dense blocks; the one-value-per-block storage (MFH_OP_MASS_VECTOR) has k_spmv_kron only");
    if (!op_batch_supported(a.dim, NR)) throw Error(MFH_ERR_UNSUPPORTED, "assembled SpMV: unsupported batch size " + std::to_string(NR));
    const int grid = persistent_grid(nList, 256 * 8);
    auto launch = [&](auto D, auto N, auto NS) {
        const size_t lds = ((size_t)a.dim * NS() * a.chunkSlots + 8) * sizeof(double);
        launch_k(k_spmv_nr<D(), N(), NS()>, dim3(grid), dim3(256), lds, s, a, x, y, dotOut, scal, it, ctl, chunkList, nList);
    };
    // the smoother of a multigrid level (FP32 copy of the matrix) takes all six vectors in ONE pass over the matrix: it is bound by the matrix bytes
    const bool onePass = a.dim == 3 && NR == 6 && a.vals32 && ((size_t)a.dim * 6 * a.chunkSlots + 8) * sizeof(double) <= 80 * 1024;
    if (onePass) launch(ic<3>{}, ic<6>{}, ic<6>{});
    else with_batch_1d(a.dim, NR, "assembled SpMV: unsupported batch size", launch);
    CHECK_LAUNCH();
}

void launch_flag_halo_blocks(int64_t nBlocks, const int32_t *blockPtr, const int32_t *entryDest, uint8_t *flag, hipStream_t s) {
    if (!nBlocks) return;
    hipLaunchKernelGGL(k_flag_halo_blocks, dim3(grid_for(nBlocks)), dim3(256), 0, s, nBlocks, blockPtr, entryDest, flag);
    CHECK_LAUNCH();
}
void launch_flag_halo_chunks(int64_t nChunk, const int32_t *chunkRow, const int32_t *rowPtr, const int32_t *colIdx, int64_t nOwnedCols, uint8_t *flag,
                             hipStream_t s) {
    if (!nChunk) return;
    hipLaunchKernelGGL(k_flag_halo_chunks, dim3(grid_for(nChunk)), dim3(256), 0, s, nChunk, chunkRow, rowPtr, colIdx, nOwnedCols, flag);
    CHECK_LAUNCH();
}

}} // namespace mfh::k
