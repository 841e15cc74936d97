// C ABI, Simulator level (include/meshfem_hip.h): boundary conditions and loads, Simulator::solve with the pin / translation
// / rotation rows of assembleConstrainedSystem, strain / stress fields, discrete shape derivatives, operator selection.
// Host orchestration only: every numeric loop runs in mfh_kernels.hip.
#include "mfh_ctx.hh"
#include <map>

using namespace mfh;
using namespace mfhi;

// K is singular on the free variables (rigid-motion constraint rows) and so are the Galerkin coarse operators: the two-level preconditioner
// steps aside for block-Jacobi; the multigrid hierarchy is rebuilt with its dense last level pinned (mfh_multigrid.cpp) and stays in use
static void singular_system_preconditioner(mfh_ctx *c) {
    c->precondNote.clear();
    if (c->precond == MFH_PRECOND_MULTIGRID) {
        ensure_precond(c);
        if (ensure_multigrid(c)) { c->precondNote = "multigrid preconditioner on a singular system (rigid-motion constraint rows): dense level pinned"; return; }
    }
    if (c->precond == MFH_PRECOND_TWO_LEVEL || c->precond == MFH_PRECOND_MULTIGRID)
        c->precondNote = "two-level / multigrid preconditioner: singular system (rigid-motion constraint rows); using block-Jacobi";
}

extern "C" {

// ---------------------------------------------------------------- Simulator-level helpers
mfh_status mfh_bc_clear(mfh_ctx *c) {
    MFH_TRY(c)
    require(c && c->haveMesh, MFH_ERR_STATE, "no mesh set");
    reset_bcs(c);
    MFH_CATCH(c)
}

mfh_status mfh_bc_dirichlet_box(mfh_ctx *c, const double *mn, const double *mx, int32_t relative, const double *value,
                                int32_t compMask) {
    MFH_TRY(c)
    require(c && c->haveMesh && c->mesh.hasTopology, MFH_ERR_STATE, "boundary conditions need mfh_mesh_build");
    const HostMesh &m = c->mesh;
    const int d = m.dim;
    double bmn[3], bmx[3];
    box_corners(c, mn, mx, relative, bmn, bmx);
    ensure_dirichlet_tables(c);
    for (size_t bi = 0; bi < m.bdryNodes.size(); ++bi) {   // LinearElasticity.hh:941-948
        const int32_t bn = m.bdryNodes[bi];
        bool in = true;
        for (int a = 0; a < d; ++a) {
            const double p = m.nodePos[(size_t)bn * d + a];
            in &= (p >= bmn[a]) && (p <= bmx[a]);
        }
        if (!in) continue;
        for (int a = 0; a < d; ++a) {   // BoundaryNode::setDirichlet :390-403
            if (!(compMask & (1 << a))) continue;
            if (!c->dirMask[bi * d + a]) {
                c->dirMask[bi * d + a] = 1;
                c->dirVal[bi * d + a] = value[a];
            } else if (c->op != MFH_OP_ELASTICITY)
                c->dirVal[bi * d + a] = value[a];   // scalar PDE: later conditions overwrite (Poisson.hh:75-83)
            else if (std::fabs(c->dirVal[bi * d + a] - value[a]) > 1e-10)
                throw Error(MFH_ERR_INVALID, "Conflicting dirichlet displacements.");
        }
    }
    MFH_CATCH(c)
}

mfh_status mfh_bc_neumann_box(mfh_ctx *c, const double *mn, const double *mx, int32_t relative, const double *value, int32_t kind) {
    MFH_TRY(c)
    require(c && c->haveMesh && c->mesh.hasTopology, MFH_ERR_STATE, "boundary conditions need mfh_mesh_build");
    const HostMesh &m = c->mesh;
    const int d = m.dim;
    double bmn[3], bmx[3];
    box_corners(c, mn, mx, relative, bmn, bmx);
    std::vector<int64_t> region;
    double area = 0;
    for (int64_t b = 0; b < m.nBE(); ++b) {   // :899-913
        double ctr[3] = {0, 0, 0};
        const int32_t *bn = &m.bdryElemNodes[(size_t)b * m.npbe];
        for (int k2 = 0; k2 < d; ++k2)
            for (int a = 0; a < d; ++a) ctr[a] += m.vertPos[(size_t)bn[k2] * d + a];
        bool in = true;
        for (int a = 0; a < d; ++a) { ctr[a] /= d; in &= (ctr[a] >= bmn[a]) && (ctr[a] <= bmx[a]); }
        if (!in) continue;
        region.push_back(b);
        area += m.bdryVol[b];
        for (int a = 0; a < d; ++a)
            c->neumannTraction[(size_t)b * d + a] = kind == MFH_NEUMANN_PRESSURE ? -value[0] * m.bdryNormal[(size_t)b * d + a] : value[a];
    }
    if (region.empty()) throw Error(MFH_ERR_INVALID, "Neumann region unmatched");
    if (kind == MFH_NEUMANN_FORCE)   // :926-931
        for (int64_t b : region)
            for (int a = 0; a < d; ++a) c->neumannTraction[(size_t)b * d + a] /= area;
    MFH_CATCH(c)
}

mfh_status mfh_bc_dirichlet_nodes(mfh_ctx *c, int64_t n, const int64_t *nodes, const double *values, int32_t compMask) {
    MFH_TRY(c)
    require(c && c->haveMesh && c->mesh.hasTopology, MFH_ERR_STATE, "boundary conditions need mfh_mesh_build");
    require(n >= 0 && (n == 0 || (nodes && values)), MFH_ERR_INVALID, "bad node list");
    const HostMesh &m = c->mesh;
    const int d = m.dim;
    // volume node -> position in mesh.bdryNodes (the index of the Dirichlet tables): sorted pairs, searched per listed node
    std::vector<std::pair<int32_t, int32_t>> bdryIndex(m.bdryNodes.size());
    for (size_t bi = 0; bi < m.bdryNodes.size(); ++bi) bdryIndex[bi] = {m.bdryNodes[bi], (int32_t)bi};
    std::sort(bdryIndex.begin(), bdryIndex.end());
    ensure_dirichlet_tables(c);
    for (int64_t k = 0; k < n; ++k) {   // LinearElasticity.hh:991-1002
        const int64_t nodeId = nodes[k];
        require(nodeId >= 0 && nodeId < m.nNode, MFH_ERR_INVALID, "node index out of bounds");
        auto itb = std::lower_bound(bdryIndex.begin(), bdryIndex.end(), std::make_pair((int32_t)nodeId, (int32_t)-1));
        if (itb == bdryIndex.end() || itb->first != (int32_t)nodeId) throw Error(MFH_ERR_INVALID, "Condition applied to non-boundary node " + std::to_string(nodeId));
        const size_t ni = (size_t)itb->second;
        for (int a = 0; a < d; ++a) {   // BoundaryNode::setDirichlet :390-403
            if (!(compMask & (1 << a))) continue;
            const double v = values[(size_t)k * d + a];
            if (!c->dirMask[(size_t)ni * d + a]) {
                c->dirMask[(size_t)ni * d + a] = 1;
                c->dirVal[(size_t)ni * d + a] = v;
            } else if (std::fabs(c->dirVal[(size_t)ni * d + a] - v) > 1e-10)
                throw Error(MFH_ERR_INVALID, "Conflicting dirichlet displacements.");
        }
    }
    MFH_CATCH(c)
}

mfh_status mfh_bc_neumann_elements(mfh_ctx *c, int64_t n, const int64_t *bdryElems, const double *tractions) {
    MFH_TRY(c)
    require(c && c->haveMesh && c->mesh.hasTopology, MFH_ERR_STATE, "boundary conditions need mfh_mesh_build");
    require(n >= 0 && (n == 0 || (bdryElems && tractions)), MFH_ERR_INVALID, "bad element list");
    const HostMesh &m = c->mesh;
    const int d = m.dim;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t b = bdryElems[k];
        require(b >= 0 && b < m.nBE(), MFH_ERR_INVALID, "boundary element index out of bounds");
        for (int a = 0; a < d; ++a) c->neumannTraction[(size_t)b * d + a] = tractions[(size_t)k * d + a];
    }
    MFH_CATCH(c)
}

mfh_status mfh_bc_delta_force(mfh_ctx *c, int64_t node, const double *force) {
    MFH_TRY(c)
    require(c && c->haveMesh && force && node >= 0 && node < c->mesh.nNode, MFH_ERR_INVALID, "bad node");
    std::array<double, 3> f{0, 0, 0};
    for (int a = 0; a < c->dim(); ++a) f[a] = force[a];
    c->deltaForces.emplace_back(node, f);
    MFH_CATCH(c)
}

mfh_status mfh_bc_dirichlet_vars(mfh_ctx *c, int64_t *vars, double *vals, int64_t *n) {
    MFH_TRY(c)
    require(c && c->haveMesh && n, MFH_ERR_STATE, "no mesh set");
    std::vector<int64_t> v;
    std::vector<double> x;
    dirichlet_vars(c, v, x);
    if (vars && vals) {
        require(*n >= (int64_t)v.size(), MFH_ERR_INVALID, "buffers too small");
        std::copy(v.begin(), v.end(), vars);
        std::copy(x.begin(), x.end(), vals);
    }
    *n = (int64_t)v.size();
    MFH_CATCH(c)
}

mfh_status mfh_pin_node(const mfh_ctx *c, int64_t *node) {
    if (!c || !c->haveMesh || !node) return MFH_ERR_STATE;
    *node = pin_node(c);
    return MFH_OK;
}

mfh_status mfh_neumann_load(mfh_ctx *c, double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && out, MFH_ERR_STATE, "no mesh set");
    const HostMesh &m = c->mesh;
    const int d = m.dim;
    parallel_ranges((int64_t)d * c->nDoF, [&](int64_t lo, int64_t hi, int) { std::fill(out + lo, out + hi, 0.0); });
    // integral of the boundary shape functions (Functions.hh:246-274): P1 1/K' each; P2 face {0,0,0,1/3,1/3,1/3};
    // P2 edge {1/6,1/6,4/6}
    double w[6] = {0, 0, 0, 0, 0, 0};
    if (m.deg == 1) for (int k2 = 0; k2 < m.npbe; ++k2) w[k2] = 1.0 / m.npbe;
    else if (d == 3) { w[3] = w[4] = w[5] = 1.0 / 3.0; }
    else { w[0] = w[1] = 1.0 / 6.0; w[2] = 4.0 / 6.0; }
    for (int64_t b = 0; b < m.nBE(); ++b)   // LinearElasticity.hh:706-710
        for (int k2 = 0; k2 < m.npbe; ++k2) {
            const int32_t dof = dof_of(c, m.bdryElemNodes[(size_t)b * m.npbe + k2]);
            for (int a = 0; a < d; ++a) out[(size_t)dof * d + a] += (w[k2] * m.bdryVol[b]) * c->neumannTraction[(size_t)b * d + a];
        }
    for (auto &df : c->deltaForces)
        for (int a = 0; a < d; ++a) out[(size_t)dof_of(c, df.first) * d + a] += df.second[a];
    MFH_CATCH(c)
}

// neumannLoad formed on the device, into c->wf -- where the solve that follows expects its right-hand side (solve_one with f == nullptr): no
// 178 MB zero fill on the host and no upload of a vector that is zero except on the loaded boundary (9 + 8 ms at configs[2]). The face loop of
// mfh_neumann_load as a kernel (VERDICT r5 missing 6); delta forces are added by a second small scatter.
static bool neumann_load_device(mfh_ctx *c) {
    const HostMesh &m = c->mesh;
    if (c->hostOnly || c->op != MFH_OP_ELASTICITY || !m.hasTopology || c->deterministic) return false;
    const int d = m.dim;
    const int64_t n = (int64_t)d * c->nDoF;
    hipStream_t s = c->stream;
    MFH_HIP(hipSetDevice(c->device));
    double w[6] = {0, 0, 0, 0, 0, 0};
    if (m.deg == 1) for (int k2 = 0; k2 < m.npbe; ++k2) w[k2] = 1.0 / m.npbe;
    else if (d == 3) { w[3] = w[4] = w[5] = 1.0 / 3.0; }
    else { w[0] = w[1] = 1.0 / 6.0; w[2] = 4.0 / 6.0; }
    // only the loaded boundary elements travel (a traction condition covers a face of the body, not its whole boundary)
    std::vector<int32_t> ben;
    std::vector<double> vol, tr;
    for (int64_t b = 0; b < m.nBE(); ++b) {
        bool any = false;
        for (int a = 0; a < d; ++a) any |= c->neumannTraction[(size_t)b * d + a] != 0.0;
        if (!any) continue;
        for (int k2 = 0; k2 < m.npbe; ++k2) ben.push_back(m.bdryElemNodes[(size_t)b * m.npbe + k2]);
        vol.push_back(m.bdryVol[b]);
        for (int a = 0; a < d; ++a) tr.push_back(c->neumannTraction[(size_t)b * d + a]);
    }
    c->wf.alloc((size_t)n);
    c->wf.zero(s);
    if (!vol.empty()) {
        DBuf<int32_t> dBen;
        DBuf<double> dVol, dTr;
        dBen.upload(ben, s); dVol.upload(vol, s); dTr.upload(tr, s);
        k::launch_neumann_load((int64_t)vol.size(), m.npbe, d, w, dBen.p, device_dof_map(c), dVol.p, dTr.p, c->wf.p, s);
        MFH_HIP(hipStreamSynchronize(s));        // (the three small buffers are released when this returns)
    }
    if (!c->deltaForces.empty()) {
        std::vector<int64_t> idx;
        std::vector<double> val;
        // several forces on one node add up (host side: a scatter kernel stores)
        std::map<int64_t, double> acc;
        for (auto &df : c->deltaForces)
            for (int a = 0; a < d; ++a) acc[(int64_t)dof_of(c, df.first) * d + a] += df.second[a];
        // forces on loaded boundary nodes must be ADDED to what the kernel wrote: read those entries back (a handful)
        for (auto &kv : acc) { idx.push_back(kv.first); val.push_back(kv.second); }
        std::vector<double> cur(idx.size());
        for (size_t q = 0; q < idx.size(); ++q) MFH_HIP(hipMemcpyAsync(&cur[q], c->wf.p + idx[q], sizeof(double), hipMemcpyDeviceToHost, s));
        MFH_HIP(hipStreamSynchronize(s));
        for (size_t q = 0; q < idx.size(); ++q) { cur[q] += val[q]; MFH_HIP(hipMemcpyAsync(c->wf.p + idx[q], &cur[q], sizeof(double), hipMemcpyHostToDevice, s)); }
        MFH_HIP(hipStreamSynchronize(s));
    }
    return true;
}

// per-vertex perturbation field on the device (shape derivatives); indexed by the node id of the element corners
static void upload_delta_p(mfh_ctx *c, const double *deltaP, DBuf<double> &buf) {
    const HostMesh &m = c->mesh;
    buf.alloc((size_t)m.nVert * m.dim);
    MFH_HIP(hipMemcpyAsync(buf.p, deltaP, (size_t)m.nVert * m.dim * sizeof(double), hipMemcpyHostToDevice, c->stream));
}

static void constant_strain_load_impl(mfh_ctx *c, const double *cstrain, const double *deltaP, double *out) {
    require(c->op == MFH_OP_ELASTICITY, MFH_ERR_STATE, "constantStrainLoad is defined for the elasticity operator");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
    const int d = c->dim();
    const int64_t n = (int64_t)d * c->nDoF;
    double cs[6] = {0, 0, 0, 0, 0, 0};
    for (int k2 = 0; k2 < flat_len(d); ++k2) cs[k2] = cstrain[k2];
    DBuf<double> dp;
    if (deltaP) upload_delta_p(c, deltaP, dp);
    c->wb.alloc(n);
    // once the matrix-free operator's lists exist the load is an application of its element routine (LDS sums, 0.25 ms at 2 M quadratic tets);
    // before that -- a caller that only wants load vectors -- the stand-alone kernel with its global atomics (2.3 ms) needs nothing but the records
    // (its LDS sums arrive in any order: not under option "deterministic")
    if (!deltaP && c->mfcValid && !c->deterministic && constant_strain_load_device(c, cs, c->wb.p)) { c->wb.download(out, (size_t)n, c->stream); return; }
    c->wb.zero(c->stream);
    k::launch_constant_strain_load(asm_args(c), c->dElemNodes.p, device_dof_map(c), c->tables.intGrad.data(), cs, deltaP ? dp.p : nullptr,
                                   c->wb.p, c->stream);
    c->wb.download(out, (size_t)n, c->stream);
}

mfh_status mfh_constant_strain_load(mfh_ctx *c, const double *cstrain, double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && cstrain && out, MFH_ERR_STATE, "no mesh set");
    constant_strain_load_impl(c, cstrain, nullptr, out);
    MFH_CATCH(c)
}

mfh_status mfh_delta_constant_strain_load(mfh_ctx *c, const double *cstrain, const double *deltaP, double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && cstrain && deltaP && out, MFH_ERR_STATE, "no mesh set");
    constant_strain_load_impl(c, cstrain, deltaP, out);
    MFH_CATCH(c)
}

mfh_status mfh_apply_delta_K(mfh_ctx *c, const double *uNodes, const double *deltaP, double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes && deltaP && out, MFH_ERR_STATE, "no mesh set");
    require(c->op == MFH_OP_ELASTICITY, MFH_ERR_STATE, "applyDeltaStiffnessMatrix is defined for the elasticity operator");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
    const HostMesh &m = c->mesh;
    const int d = m.dim;
    const int64_t n = (int64_t)d * c->nDoF;
    DBuf<double> dp, u;
    upload_delta_p(c, deltaP, dp);
    u.alloc((size_t)m.nNode * d);
    MFH_HIP(hipMemcpyAsync(u.p, uNodes, (size_t)m.nNode * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->wb.alloc(n);
    c->wb.zero(c->stream);
    k::launch_apply_delta_K(asm_args(c), c->dElemNodes.p, device_dof_map(c), c->tables.intGrad.data(), u.p, dp.p, c->wb.p, c->stream);
    c->wb.download(out, (size_t)n, c->stream);
    MFH_CATCH(c)
}

mfh_status mfh_mutual_energies(mfh_ctx *c, const double *w, const double *deltaP, double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && w && out, MFH_ERR_STATE, "no mesh set");
    require(c->op == MFH_OP_ELASTICITY, MFH_ERR_STATE, "mutual energies are defined for the elasticity operator");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
    const HostMesh &m = c->mesh;
    const int d = m.dim, fl = flat_len(d), np = fl * (fl + 1) / 2;
    DBuf<double> dp, wd, res;
    if (deltaP) upload_delta_p(c, deltaP, dp);
    wd.alloc((size_t)fl * m.nNode * d);
    MFH_HIP(hipMemcpyAsync(wd.p, w, wd.n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    res.alloc(np);
    res.zero(c->stream);
    k::launch_mutual_energies(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), wd.p, m.nNode, deltaP ? dp.p : nullptr, res.p, c->stream);
    std::vector<double> h(np);
    res.download(h.data(), (size_t)np, c->stream);
    int p = 0;
    for (int i = 0; i < fl; ++i)
        for (int j = i; j < fl; ++j, ++p) out[i * fl + j] = out[j * fl + i] = h[p];
    MFH_CATCH(c)
}

// ---- small dense helpers for the constraint rows (k <= 6)
static bool dense_solve(int k, std::vector<double> A /* k x k row-major */, std::vector<double> &b) {
    for (int col = 0; col < k; ++col) {
        int piv = col;
        for (int r = col + 1; r < k; ++r)
            if (std::fabs(A[(size_t)r * k + col]) > std::fabs(A[(size_t)piv * k + col])) piv = r;
        if (!(std::fabs(A[(size_t)piv * k + col]) > 0)) return false;
        if (piv != col) {
            for (int q = 0; q < k; ++q) std::swap(A[(size_t)piv * k + q], A[(size_t)col * k + q]);
            std::swap(b[piv], b[col]);
        }
        for (int r = col + 1; r < k; ++r) {
            const double fct = A[(size_t)r * k + col] / A[(size_t)col * k + col];
            for (int q = col; q < k; ++q) A[(size_t)r * k + q] -= fct * A[(size_t)col * k + q];
            b[r] -= fct * b[col];
        }
    }
    for (int r = k - 1; r >= 0; --r) {
        double v = b[r];
        for (int q = r + 1; q < k; ++q) v -= A[(size_t)r * k + q] * b[q];
        b[r] = v / A[(size_t)r * k + r];
    }
    return true;
}
// cyclic Jacobi eigen-decomposition of a small symmetric matrix: A -> eigenvalues on the diagonal, V columns = eigenvectors
static void jacobi_eig(int k, std::vector<double> &A, std::vector<double> &V) {
    V.assign((size_t)k * k, 0.0);
    for (int q = 0; q < k; ++q) V[(size_t)q * k + q] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0;
        for (int p2 = 0; p2 < k; ++p2)
            for (int q = p2 + 1; q < k; ++q) off += A[(size_t)p2 * k + q] * A[(size_t)p2 * k + q];
        if (off < 1e-300) break;
        for (int p2 = 0; p2 < k; ++p2)
            for (int q = p2 + 1; q < k; ++q) {
                const double apq = A[(size_t)p2 * k + q];
                if (std::fabs(apq) < 1e-300) continue;
                const double th = (A[(size_t)q * k + q] - A[(size_t)p2 * k + p2]) / (2 * apq);
                const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1));
                const double cs = 1 / std::sqrt(t * t + 1), sn = t * cs;
                for (int r = 0; r < k; ++r) {
                    const double arp = A[(size_t)r * k + p2], arq = A[(size_t)r * k + q];
                    A[(size_t)r * k + p2] = cs * arp - sn * arq; A[(size_t)r * k + q] = sn * arp + cs * arq;
                }
                for (int r = 0; r < k; ++r) {
                    const double apr = A[(size_t)p2 * k + r], aqr = A[(size_t)q * k + r];
                    A[(size_t)p2 * k + r] = cs * apr - sn * aqr; A[(size_t)q * k + r] = sn * apr + cs * aqr;
                }
                for (int r = 0; r < k; ++r) {
                    const double vrp = V[(size_t)r * k + p2], vrq = V[(size_t)r * k + q];
                    V[(size_t)r * k + p2] = cs * vrp - sn * vrq; V[(size_t)r * k + q] = sn * vrp + cs * vrq;
                }
            }
    }
}
// y += a x and y *= a on all host threads (the constraint rows and rigid modes are full-length vectors: tens of them at 20 M DoFs)
static void paxpy_n(double *yp, double a, const double *xp, int64_t n) {
    parallel_ranges(n, [&](int64_t lo, int64_t hi, int) { for (int64_t q = lo; q < hi; ++q) yp[q] += a * xp[q]; });
}
static void paxpy(std::vector<double> &y, double a, const std::vector<double> &x) { paxpy_n(y.data(), a, x.data(), (int64_t)y.size()); }
static void paxpy(RawVec<double> &y, double a, const std::vector<double> &x) { paxpy_n(y.data(), a, x.data(), (int64_t)y.size()); }
static void pscale(std::vector<double> &y, double a) {
    double *yp = y.data();
    parallel_ranges((int64_t)y.size(), [&](int64_t lo, int64_t hi, int) { for (int64_t q = lo; q < hi; ++q) yp[q] *= a; });
}
static double hdot_n(const double *a, const double *b, int64_t n) {
    const int nt = host_threads();
    std::vector<double> part((size_t)nt + 1, 0.0);
    parallel_ranges(n, [&](int64_t lo, int64_t hi, int tid) {
        double v = 0;
        for (int64_t q = lo; q < hi; ++q) v += a[q] * b[q];
        part[tid] += v;
    });
    double v = 0;
    for (double x : part) v += x;
    return v;
}
static double hdot(const std::vector<double> &a, const std::vector<double> &b) { return hdot_n(a.data(), b.data(), (int64_t)a.size()); }
static double hdot(const std::vector<double> &a, const RawVec<double> &b) { return hdot_n(a.data(), b.data(), (int64_t)a.size()); }

// Simulator::solve with the whole of assembleConstrainedSystem (LinearElasticity.hh:1201-1249): pin / translation /
// rotation constraints, Dirichlet variables. The reference solves the resulting KKT system with UMFPACK
// (SparseMatrices.hh:2572-2590); here the constraint rows C (k <= 6) are eliminated around SPD solves:
//   * K singular on the free variables with null space Z (rigid motions vanishing on the fixed variables) and
//     C Z square and regular: multipliers from Z^T (f - C^T l) = 0, ONE consistent singular PCG solve, rigid part of the
//     solution from C u = c;
//   * K regular on the free variables: Schur complement S = C K^-1 C^T with k + 1 PCG solves.
// nrhs > 1 (mfh_sim_solve_batch): f / uNodes / info hold nrhs right-hand sides; systems that need constraint rows are refused (the caller
// then solves one right-hand side after the other)
// cstrains != null (mfh_solve_cell_problems): the nrhs right-hand sides are constantStrainLoad(cstrains[r]); f is not read
static void sim_solve_impl(mfh_ctx *c, const double *f, int32_t flags, const double *rmRHS, int32_t nRM, double *uNodes, double rtol,
                           int32_t maxit, mfh_solve_info *info, int nrhs = 1, const double *cstrains = nullptr) {
    const HostMesh &m = c->mesh;
    const int d = c->bs(), gd = m.dim;
    const int64_t n = (int64_t)d * c->nDoF;
    if (c->op != MFH_OP_ELASTICITY) flags = MFH_SOLVE_ALLOW_ILL_POSED;   // rigid motions are an elasticity notion
    const bool periodic = !c->dofForNode.empty();
    // MFH_SOLVE_TIMING=1: host-side laps of one Simulator::solve on stderr (the device part is in mfh_solve_info)
    const bool lapTiming = getenv("MFH_SOLVE_TIMING") != nullptr;
    double lapT = now_ms();
    auto lap = [&](const char *what) {
        if (!lapTiming) return;
        const double t = now_ms();
        fprintf(stderr, "[mfh solve] %-32s %8.2f ms\n", what, t - lapT);
        lapT = t;
    };
    std::vector<int64_t> vars;
    std::vector<double> vals;
    std::vector<std::vector<double>> C;
    std::vector<double> crhs;
    auto pin = [&](unsigned compMask) {   // m_pinNode (:1595-1618)
        const int64_t pn = pin_node(c);
        for (int a = 0; a < d; ++a)
            if (compMask & (1u << a)) { vars.push_back((int64_t)d * dof_of(c, pn) + a); vals.push_back(0.0); }
    };
    auto addTranslationRows = [&](unsigned compMask) {   // m_appendTranslationMatrix (:1568-1590)
        for (int a = 0; a < d; ++a) {
            if (!(compMask & (1u << a))) continue;
            std::vector<double> row((size_t)n);
            double *rp = row.data();
            parallel_ranges(c->nDoF, [&](int64_t lo, int64_t hi, int) {
                for (int64_t i = lo; i < hi; ++i)
                    for (int b = 0; b < d; ++b) rp[(size_t)i * d + b] = b == a ? 1.0 : 0.0;
            });
            C.push_back(std::move(row));
        }
    };
    auto rotationRows = [&](std::vector<std::vector<double>> &out) {   // rows of m_appendInfinitesimalRotationMatrix (:1525-1566)
        const int nr = gd == 3 ? 3 : 1;
        for (int r = 0; r < nr; ++r) out.emplace_back((size_t)n, 0.0);
        std::vector<double> *R = &out[out.size() - nr];
        parallel_ranges(m.nNode, [&](int64_t lo, int64_t hi, int) {
            for (int64_t k2 = lo; k2 < hi; ++k2) {
                const double *x = &m.nodePos[(size_t)k2 * gd];
                if (gd == 3) {
                    R[0][(size_t)k2 * 3 + 1] = -x[2]; R[0][(size_t)k2 * 3 + 2] = x[1];
                    R[1][(size_t)k2 * 3 + 0] = x[2];  R[1][(size_t)k2 * 3 + 2] = -x[0];
                    R[2][(size_t)k2 * 3 + 0] = -x[1]; R[2][(size_t)k2 * 3 + 1] = x[0];
                } else {
                    R[0][(size_t)k2 * 2 + 0] = -x[1]; R[0][(size_t)k2 * 2 + 1] = x[0];
                }
            }
        });
    };
    const unsigned allComps = (1u << d) - 1;
    if (flags & MFH_SOLVE_NO_RIGID_MOTION) {
        // periodic conditions pin the rotations (:1534-1542)
        bool rot = true;
        if (gd == 2 && c->nDoF < m.nNode) rot = false;
        else if (c->nDoF < m.nNode - 1) rot = false;
        else if (c->nDoF < m.nNode) throw Error(MFH_ERR_UNSUPPORTED, "Single pair periodic BC unsupported in 3D.");
        if (rot) rotationRows(C);
        if (flags & MFH_SOLVE_PIN) pin(allComps);
        else addTranslationRows(allComps);
        if (rmRHS && nRM > 0) {
            require((size_t)nRM == C.size(), MFH_ERR_INVALID, "Invalid rigid motion RHS");
            crhs.assign(rmRHS, rmRHS + nRM);
        } else crhs.assign(C.size(), 0.0);
    } else if (!(flags & MFH_SOLVE_ALLOW_ILL_POSED)) {
        // analyzeDirichletPosedness (:1169-1190)
        unsigned needsT = allComps;
        size_t total = 0;
        for (size_t bi = 0; bi < m.bdryNodes.size(); ++bi)
            for (int a = 0; a < gd; ++a)
                if (!c->dirMask.empty() && c->dirMask[bi * gd + a]) { needsT &= ~(1u << a); ++total; }
        if (needsT) {
            if (flags & MFH_SOLVE_PIN) pin(needsT);
            else { addTranslationRows(needsT); crhs.assign(C.size(), 0.0); }
        }
        if (total == 0) throw Error(MFH_ERR_UNSUPPORTED, "Unimplemented");   // needsRotations (:1240): ask for the rigid-motion constraint
    }
    dirichlet_vars(c, vars, vals);
    lap("constraint rows + Dirichlet vars");
    if (vars != c->fixedVars || vals != c->fixedVals) {   // unchanged constraints keep the preconditioner setup
        clear_fixed(c);
        add_fixed(c, (int64_t)vars.size(), vars.data(), vals.data());
    }
    lap("fixed-variable mask");
    // host scratch vectors live in the context: a fresh 178 MB std::vector costs ~30 ms of page faults per solve at config 3
    RawVec<double> &load = c->hLoad;
    // Simulator::solve() without a load vector = solve(neumannLoad()) (LinearElasticity.hh:657): where nothing on the host needs the vector --
    // a positive definite system, the classic loop -- it is formed on the device, where the solve wants it (f stays null: solve_one reads c->wf)
    const bool loadOnDevice = !f && nrhs == 1 && C.empty() && device_rhs_supported(c) && c->deltaForces.size() <= 64 && neumann_load_device(c);
    if (loadOnDevice) lap("load vector (device)");
    if (!f && !loadOnDevice) {
        resize_prefaulted(load, (size_t)n);
        if (c->op == MFH_OP_ELASTICITY) {
            mfh_status st = mfh_neumann_load(c, load.data());   // zero-fills first
            if (st != MFH_OK) throw Error(st, c->err);
        } else parallel_ranges(n, [&](int64_t lo, int64_t hi, int) { std::fill(load.data() + lo, load.data() + hi, 0.0); });   // scalar PDE: zero right-hand side, zero-Neumann natural condition (Poisson.hh:100-102)
        f = load.data();
    }
    lap("load vector");
    RawVec<double> &x = c->hX;
    resize_prefaulted(x, (size_t)n);
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_precond(c);
    lap("assembly + diagonal blocks");
    // the multigrid hierarchy depends on whether the solve ahead is singular (pinned dense level): it is built where that is known -- right
    // before the first solve_one of the branch taken (solve_one makes sure of it) -- instead of here and then again
    if (c->precond != MFH_PRECOND_MULTIGRID) ensure_coarse_levels(c, 1);
    lap("two-level setup");
    mfh_solve_info li{};
    const int k = (int)C.size();
    if (nrhs > 1) {
        if (k != 0 || (!f && !cstrains)) throw Error(MFH_ERR_UNSUPPORTED, "batched Simulator::solve: the system needs constraint rows");
        const int64_t nn = m.nNode * d;
        if (cstrains) {
            // loads formed on the device, solutions downloaded as nodal fields: no host copy of a load or of a DoF vector exists
            const int fl = flat_len(gd);
            if (!multigrid_batch_ready(c, nrhs)) throw Error(MFH_ERR_UNSUPPORTED, "batched cell problems: the batched V-cycle does not apply to this context");
            int r0 = 0;
            bool all = true;
            std::vector<mfh_solve_info> lis((size_t)nrhs);
            while (r0 < nrhs) {
                int nb = 1;
                for (int cand : {6, 3, 2})
                    if (cand <= nrhs - r0 && k::op_batch_supported(d, cand)) { nb = cand; break; }
                if (nb == 1) throw Error(MFH_ERR_UNSUPPORTED, "batched cell problems: right-hand sides left over");   // (3 / 6 strains fill their batches)
                BatchIO io;
                io.cstrains = cstrains + (size_t)r0 * fl; io.uNodes = uNodes + (size_t)r0 * nn; io.nodeStride = nn;
                solve_multigrid_batch(c, nb, nullptr, nullptr, 0, rtol, maxit, lis.data() + r0, &io);
                r0 += nb;
            }
            lap("PCG incl. loads and downloads (batch, device-resident)");
            for (int r = 0; r < nrhs; ++r) {
                // (a solve that needs iterative refinement -- true residual above twice the tolerance: rare -- is redone the long way)
                if (c->refine && rtol > 0 && lis[(size_t)r].converged && lis[(size_t)r].true_rel_residual > 2.0 * rtol && lis[(size_t)r].true_rel_residual < 1.0) {
                    resize_prefaulted(c->hLoad, (size_t)n);
                    constant_strain_load_impl(c, cstrains + (size_t)r * fl, nullptr, c->hLoad.data());
                    solve_one(c, c->hLoad.data(), x.data(), rtol, maxit, &lis[(size_t)r]);
                    for (int64_t i = 0; i < m.nNode; ++i)
                        for (int a = 0; a < d; ++a) uNodes[(size_t)r * nn + (size_t)i * d + a] = x[(size_t)dof_of(c, i) * d + a];
                }
                if (info) info[r] = lis[(size_t)r];
                all = all && lis[(size_t)r].converged;
            }
            if (!all) throw Error(MFH_ERR_NOT_CONVERGED, "PCG did not reach the requested tolerance within maxit iterations");
            return;
        }
        RawVec<double> &xs = c->hXBatch;
        resize_prefaulted(xs, (size_t)n * nrhs);
        std::vector<mfh_solve_info> lis((size_t)nrhs);
        solve_many(c, nrhs, f, xs.data(), n, rtol, maxit, lis.data());
        lap("PCG incl. transfers (batch)");
        bool all = true;
        for (int r = 0; r < nrhs; ++r) { if (info) info[r] = lis[(size_t)r]; all = all && lis[(size_t)r].converged; }
        parallel_ranges(m.nNode, [&](int64_t nb, int64_t ne, int) {   // dofToNodeField :664-677
            for (int r = 0; r < nrhs; ++r)
                for (int64_t i = nb; i < ne; ++i)
                    for (int a = 0; a < d; ++a) uNodes[(size_t)r * nn + (size_t)i * d + a] = xs[(size_t)r * n + (size_t)dof_of(c, i) * d + a];
        });
        lap("dofToNodeField");
        if (!all) throw Error(MFH_ERR_NOT_CONVERGED, "PCG did not reach the requested tolerance within maxit iterations");
        return;
    }
    if (k == 0) {
        solve_one(c, f, x.data(), rtol, maxit, &li);
        lap("PCG incl. transfers");
    } else {
        // ---- candidate rigid motions (unit-normalised): translations, and rotations unless a periodic map excludes them
        std::vector<std::vector<double>> Zc;
        for (int a = 0; a < d; ++a) {
            Zc.emplace_back((size_t)n);
            double *zp = Zc.back().data();
            parallel_ranges(c->nDoF, [&](int64_t lo, int64_t hi, int) {
                for (int64_t i = lo; i < hi; ++i)
                    for (int b = 0; b < d; ++b) zp[(size_t)i * d + b] = b == a ? 1.0 : 0.0;
            });
        }
        if (!periodic) rotationRows(Zc);
        const int nc = (int)Zc.size();
        for (auto &z : Zc) {
            const double nrm = std::sqrt(hdot(z, z));
            if (nrm > 0) pscale(z, 1.0 / nrm);
        }
        // null space of the candidates restricted to the fixed variables
        std::vector<double> G((size_t)nc * nc, 0.0), V;
        for (int64_t fv : c->fixedVars)
            for (int a = 0; a < nc; ++a)
                for (int b = 0; b < nc; ++b) G[(size_t)a * nc + b] += Zc[a][(size_t)fv] * Zc[b][(size_t)fv];
        jacobi_eig(nc, G, V);
        double evMax = 0;
        for (int e = 0; e < nc; ++e) evMax = std::max(evMax, G[(size_t)e * nc + e]);
        std::vector<std::vector<double>> Z;
        if (c->fixedVars.empty()) Z = std::move(Zc);               // nothing is fixed: every candidate is a null vector as it stands
        else
        for (int e = 0; e < nc; ++e) {
            if (G[(size_t)e * nc + e] > 1e-12 * evMax) continue;   // the mode moves a fixed variable: not in the null space
            Z.emplace_back((size_t)n, 0.0);
            for (int a = 0; a < nc; ++a) {
                const double w = V[(size_t)a * nc + e];
                if (w == 0.0) continue;
                paxpy(Z.back(), w, Zc[a]);
            }
            for (int64_t fv : c->fixedVars) Z.back()[(size_t)fv] = 0.0;
        }
        std::vector<std::vector<double>>().swap(Zc);
        const int q = (int)Z.size();
        // constraint rows on the free variables
        std::vector<std::vector<double>> CfStore;
        if (!c->fixedVars.empty()) {
            CfStore = C;
            for (auto &row : CfStore)
                for (int64_t fv : c->fixedVars) row[(size_t)fv] = 0.0;
        }
        const std::vector<std::vector<double>> &Cf = c->fixedVars.empty() ? C : CfStore;   // (full-length vectors: no copy without a reason)
        if (q == k) {
            std::vector<double> M((size_t)k * k), MT((size_t)k * k);
            for (int r = 0; r < k; ++r)
                for (int e = 0; e < k; ++e) { M[(size_t)r * k + e] = hdot(Cf[r], Z[e]); MT[(size_t)e * k + r] = M[(size_t)r * k + e]; }
            std::vector<double> lam((size_t)k), fv2(f, f + n);
            for (int e = 0; e < k; ++e) lam[e] = hdot(Z[e], fv2);
            if (!dense_solve(k, MT, lam)) throw Error(MFH_ERR_UNSUPPORTED, "constraint rows do not fix the rigid motions of the system");
            for (int r = 0; r < k; ++r) paxpy(fv2, -lam[r], Cf[r]);
            // K is singular on the free variables, and so is the Galerkin coarse operator of the two-level
            // preconditioner (the aggregates' modes span the global rigid motions): block-Jacobi for this solve
            c->tlSuppress = true;
            singular_system_preconditioner(c);
            try { solve_one(c, fv2.data(), x.data(), rtol, maxit, &li); } catch (...) { c->tlSuppress = false; throw; }
            c->tlSuppress = false;
            std::vector<double> a((size_t)k);
            for (int r = 0; r < k; ++r) a[r] = crhs[r] - hdot(C[r], x);
            if (!dense_solve(k, M, a)) throw Error(MFH_ERR_UNSUPPORTED, "constraint rows do not fix the rigid motions of the system");
            for (int e = 0; e < k; ++e) paxpy(x, a[e], Z[e]);
        } else if (q == 0) {
            solve_one(c, f, x.data(), rtol, maxit, &li);
            std::vector<std::vector<double>> Y((size_t)k, std::vector<double>((size_t)n));
            c->solveHomogeneous = true;
            try {
                for (int r = 0; r < k; ++r) {
                    mfh_solve_info lj{};
                    solve_one(c, Cf[r].data(), Y[r].data(), rtol, maxit, &lj);
                    li.iterations += lj.iterations;
                    li.solve_ms += lj.solve_ms;
                    li.converged = li.converged && lj.converged;
                }
            } catch (...) { c->solveHomogeneous = false; throw; }
            c->solveHomogeneous = false;
            std::vector<double> S((size_t)k * k), lam((size_t)k);
            for (int r = 0; r < k; ++r) {
                for (int e = 0; e < k; ++e) S[(size_t)r * k + e] = hdot(Cf[r], Y[e]);
                lam[r] = hdot(C[r], x) - crhs[r];
            }
            if (!dense_solve(k, S, lam)) throw Error(MFH_ERR_UNSUPPORTED, "constraint rows are linearly dependent on the free variables");
            for (int r = 0; r < k; ++r)
                for (int64_t i = 0; i < n; ++i) x[(size_t)i] -= lam[r] * Y[r][(size_t)i];
        } else if (q < k) {
            // Mixed case (e.g. x-displacements fixed on a face + translation rows for y and z: the rotation about x survives
            // as well, q = 3 null modes for k = 2 ... or more rows than null modes): the KKT system is regular iff B = C Z has full
            // column rank. With lambda = lambda0 + N mu (B^T lambda0 = Z^T f, N = null(B^T)) every right-hand side below is
            // consistent with the singular K:  u = K^+(f - C^T lambda0) - sum_j mu_j K^+ C^T N_j + Z a,  and (mu, a) follow from
            // C u = c. (k - q) + 1 PCG solves; reduces to the two branches above for q == k and q == 0.
            std::vector<double> B((size_t)k * q);
            for (int r = 0; r < k; ++r)
                for (int e = 0; e < q; ++e) B[(size_t)r * q + e] = hdot(Cf[r], Z[e]);
            std::vector<double> BtB((size_t)q * q, 0.0), rhsq((size_t)q), fv2(f, f + n);
            for (int e = 0; e < q; ++e) {
                rhsq[e] = hdot(Z[e], fv2);
                for (int g = 0; g < q; ++g)
                    for (int r = 0; r < k; ++r) BtB[(size_t)e * q + g] += B[(size_t)r * q + e] * B[(size_t)r * q + g];
            }
            if (!dense_solve(q, BtB, rhsq))
                throw Error(MFH_ERR_UNSUPPORTED, "constraint rows do not fix the " + std::to_string(q) + " rigid motions the fixed variables leave free");
            std::vector<double> lam0((size_t)k, 0.0);
            for (int r = 0; r < k; ++r)
                for (int e = 0; e < q; ++e) lam0[r] += B[(size_t)r * q + e] * rhsq[e];
            // N: eigenvectors of B B^T with eigenvalue 0 (k - q of them)
            std::vector<double> BBt((size_t)k * k, 0.0), Vn;
            for (int r = 0; r < k; ++r)
                for (int t2 = 0; t2 < k; ++t2)
                    for (int e = 0; e < q; ++e) BBt[(size_t)r * k + t2] += B[(size_t)r * q + e] * B[(size_t)t2 * q + e];
            jacobi_eig(k, BBt, Vn);
            double evm = 0;
            for (int e = 0; e < k; ++e) evm = std::max(evm, BBt[(size_t)e * k + e]);
            std::vector<int> nullCols;
            for (int e = 0; e < k; ++e)
                if (BBt[(size_t)e * k + e] <= 1e-12 * evm) nullCols.push_back(e);
            if ((int)nullCols.size() != k - q)
                throw Error(MFH_ERR_UNSUPPORTED, "constraint rows do not fix the " + std::to_string(q) + " rigid motions the fixed variables leave free");
            const int nm = k - q;
            for (int r = 0; r < k; ++r)
                for (int64_t i = 0; i < n; ++i) fv2[(size_t)i] -= lam0[r] * Cf[r][(size_t)i];
            c->tlSuppress = true;
            singular_system_preconditioner(c);
            std::vector<std::vector<double>> Y((size_t)nm, std::vector<double>((size_t)n));
            try {
                solve_one(c, fv2.data(), x.data(), rtol, maxit, &li);
                c->solveHomogeneous = true;
                std::vector<double> rhs((size_t)n);
                for (int j = 0; j < nm; ++j) {
                    std::fill(rhs.begin(), rhs.end(), 0.0);
                    for (int r = 0; r < k; ++r) {
                        const double w = Vn[(size_t)r * k + nullCols[j]];
                        if (w == 0.0) continue;
                        for (int64_t i = 0; i < n; ++i) rhs[(size_t)i] += w * Cf[r][(size_t)i];
                    }
                    mfh_solve_info lj{};
                    solve_one(c, rhs.data(), Y[j].data(), rtol, maxit, &lj);
                    li.iterations += lj.iterations;
                    li.solve_ms += lj.solve_ms;
                    li.converged = li.converged && lj.converged;
                }
            } catch (...) { c->solveHomogeneous = false; c->tlSuppress = false; throw; }
            c->solveHomogeneous = false;
            c->tlSuppress = false;
            std::vector<double> S((size_t)k * k), un((size_t)k);
            for (int r = 0; r < k; ++r) {
                for (int j = 0; j < nm; ++j) S[(size_t)r * k + j] = -hdot(Cf[r], Y[j]);
                for (int e = 0; e < q; ++e) S[(size_t)r * k + nm + e] = B[(size_t)r * q + e];
                un[r] = crhs[r] - hdot(C[r], x);
            }
            if (!dense_solve(k, S, un)) throw Error(MFH_ERR_UNSUPPORTED, "constraint rows are linearly dependent on the free variables");
            for (int j = 0; j < nm; ++j)
                for (int64_t i = 0; i < n; ++i) x[(size_t)i] -= un[j] * Y[j][(size_t)i];
            for (int e = 0; e < q; ++e)
                for (int64_t i = 0; i < n; ++i) x[(size_t)i] += un[nm + e] * Z[e][(size_t)i];
        } else
            throw Error(MFH_ERR_UNSUPPORTED, "the fixed variables leave " + std::to_string(q) + " rigid motions free but there are only " + std::to_string(k) +
                                                 " constraint rows: the system is singular (add no_rigid_motion or pin more nodes)");
    }
    if (info) *info = li;
    parallel_ranges(m.nNode, [&](int64_t nb, int64_t ne, int) {   // dofToNodeField :664-677
        for (int64_t i = nb; i < ne; ++i)
            for (int a = 0; a < d; ++a) uNodes[(size_t)i * d + a] = x[(size_t)dof_of(c, i) * d + a];
    });
    lap("dofToNodeField");
    if (!li.converged) throw Error(MFH_ERR_NOT_CONVERGED, "PCG did not reach the requested tolerance within maxit iterations");
}

mfh_status mfh_sim_solve(mfh_ctx *c, const double *f, int32_t usePin, double *uNodes, double rtol, int32_t maxit,
                         mfh_solve_info *info) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes, MFH_ERR_STATE, "no mesh set");
    // usePin = solveCellProblems' configuration (PeriodicHomogenization.hh:43-45): rigid-motion constraint with the
    // translations pinned; otherwise the Dirichlet variables alone
    sim_solve_impl(c, f, usePin ? (MFH_SOLVE_PIN | MFH_SOLVE_NO_RIGID_MOTION) : MFH_SOLVE_ALLOW_ILL_POSED, nullptr, 0, uNodes, rtol, maxit, info);
    MFH_CATCH(c)
}

mfh_status mfh_sim_solve_constrained(mfh_ctx *c, const double *f, int32_t flags, const double *rigidMotionRHS, int32_t nRigidRHS,
                                     double *uNodes, double rtol, int32_t maxit, mfh_solve_info *info) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes, MFH_ERR_STATE, "no mesh set");
    require(c->mesh.nOwned == c->mesh.nNode, MFH_ERR_UNSUPPORTED, "constrained solves need all rows owned");
    sim_solve_impl(c, f, flags, rigidMotionRHS, nRigidRHS, uNodes, rtol, maxit, info);
    MFH_CATCH(c)
}

mfh_status mfh_sim_solve_batch(mfh_ctx *c, int32_t nrhs, const double *f, int32_t flags, double *uNodes, double rtol, int32_t maxit,
                               mfh_solve_info *info) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes && f && nrhs >= 1, MFH_ERR_INVALID, "bad arguments");
    require(c->mesh.nOwned == c->mesh.nNode, MFH_ERR_UNSUPPORTED, "constrained solves need all rows owned");
    bool batched = false;
    if (nrhs > 1) {
        try { sim_solve_impl(c, f, flags, nullptr, 0, uNodes, rtol, maxit, info, nrhs); batched = true; }
        catch (const Error &e) { if (e.code != MFH_ERR_UNSUPPORTED) throw; }
    }
    if (!batched) {
        const int64_t n = (int64_t)c->bs() * c->nDoF, nn = c->mesh.nNode * (int64_t)c->bs();
        for (int r = 0; r < nrhs; ++r) sim_solve_impl(c, f + (size_t)r * n, flags, nullptr, 0, uNodes + (size_t)r * nn, rtol, maxit, info ? info + r : nullptr);
    }
    MFH_CATCH(c)
}

mfh_status mfh_solve_cell_problems(mfh_ctx *c, int32_t nStrains, const double *cstrains, int32_t flags, double *wNodes, double rtol, int32_t maxit,
                                   mfh_solve_info *info) {
    MFH_TRY(c)
    require(c && c->haveMesh && cstrains && wNodes && nStrains >= 1, MFH_ERR_INVALID, "bad arguments");
    require(c->mesh.nOwned == c->mesh.nNode, MFH_ERR_UNSUPPORTED, "constrained solves need all rows owned");
    require(c->op == MFH_OP_ELASTICITY, MFH_ERR_STATE, "constantStrainLoad is defined for the elasticity operator");
    bool done = false;
    if (nStrains > 1) {
        try { sim_solve_impl(c, nullptr, flags, nullptr, 0, wNodes, rtol, maxit, info, nStrains, cstrains); done = true; }
        catch (const Error &e) { if (e.code != MFH_ERR_UNSUPPORTED) throw; }
    }
    if (!done) {
        // the general route: host load vectors, right-hand sides in the batches of mfh_sim_solve_batch (or one after the other under constraint rows)
        const int fl = flat_len(c->dim());
        const int64_t n = (int64_t)c->bs() * c->nDoF, nn = c->mesh.nNode * (int64_t)c->bs();
        RawVec<double> &F = c->hLoadBatch;
        resize_prefaulted(F, (size_t)n * nStrains);
        for (int r = 0; r < nStrains; ++r) constant_strain_load_impl(c, cstrains + (size_t)r * fl, nullptr, F.data() + (size_t)r * n);
        bool batched = false;
        if (nStrains > 1) {
            try { sim_solve_impl(c, F.data(), flags, nullptr, 0, wNodes, rtol, maxit, info, nStrains); batched = true; }
            catch (const Error &e) { if (e.code != MFH_ERR_UNSUPPORTED) throw; }
        }
        if (!batched)
            for (int r = 0; r < nStrains; ++r) sim_solve_impl(c, F.data() + (size_t)r * n, flags, nullptr, 0, wNodes + (size_t)r * nn, rtol, maxit, info ? info + r : nullptr);
    }
    MFH_CATCH(c)
}

mfh_status mfh_strain_field(mfh_ctx *c, const double *uNodes, int32_t wantStress, double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes && out, MFH_ERR_STATE, "no mesh set");
    require(c->op == MFH_OP_ELASTICITY, MFH_ERR_STATE, "strain / stress fields are defined for the elasticity operator");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
    const HostMesh &m = c->mesh;
    const int d = m.dim, fl = flat_len(d), nq = m.deg == 1 ? 1 : d + 1;
    DBuf<double> u, res;
    u.alloc((size_t)m.nNode * d);
    MFH_HIP(hipMemcpyAsync(u.p, uNodes, (size_t)m.nNode * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    res.alloc((size_t)m.nElem * nq * fl);
    k::launch_strain_field(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), u.p, wantStress, res.p, c->stream);
    res.download(out, res.n, c->stream);
    MFH_CATCH(c)
}

mfh_status mfh_boundary_strain_field(mfh_ctx *c, const double *uNodes, int32_t wantStress, double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes && out, MFH_ERR_STATE, "no mesh set");
    require(c->mesh.hasTopology, MFH_ERR_STATE, "boundary elements need a mesh built with mfh_mesh_build");
    require(c->op == MFH_OP_ELASTICITY, MFH_ERR_STATE, "strain / stress fields are defined for the elasticity operator");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
    const HostMesh &m = c->mesh;
    const int d = m.dim, fl = flat_len(d), nq = m.deg == 1 ? 1 : d;
    const int64_t nBE = m.nBE();
    DBuf<double> u, res;
    DBuf<int32_t> parent, ben;
    u.alloc((size_t)m.nNode * d);
    MFH_HIP(hipMemcpyAsync(u.p, uNodes, (size_t)m.nNode * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    parent.upload(m.bdryParent, c->stream);
    ben.upload(m.bdryElemNodes, c->stream);
    res.alloc((size_t)nBE * nq * fl);
    k::launch_boundary_strain_field(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), nBE, parent.p, ben.p, m.npbe, u.p,
                                    wantStress, res.p, c->stream);
    res.download(out, res.n, c->stream);
    MFH_CATCH(c)
}

// ---- stress measures: von Mises, principal values, vertex averages, peak (docs/design/04_10_stress_measures.md)
namespace {
// an input array as the kernels read it: the caller's device pointer, or a device copy of its host array
struct DevInput {
    DBuf<double> buf;
    const double *p = nullptr;
    DevInput(const double *src, size_t n, bool onDevice, hipStream_t s) {
        if (onDevice) { p = src; return; }
        buf.alloc(n);
        if (n) MFH_HIP(hipMemcpyAsync(buf.p, src, n * sizeof(double), hipMemcpyHostToDevice, s));
        p = buf.p;
    }
};
// an output array: the caller's device pointer, or a device buffer downloaded by finish() (null when not requested)
struct DevOutput {
    DBuf<double> buf;
    double *p = nullptr, *host = nullptr;
    DevOutput(double *dst, size_t n, bool wanted, bool onDevice) {
        if (!wanted) return;
        if (onDevice) { p = dst; return; }
        buf.alloc(n);
        p = buf.p; host = dst;
    }
    void finish(hipStream_t s) { if (host) buf.download(host, buf.n, s); }
};
void require_measure_outputs(int32_t what, const double *vm, const double *eval, const double *evec) {
    require(what > 0 && what < 8, MFH_ERR_INVALID, "what: a mask of MFH_MEASURE_VON_MISES | MFH_MEASURE_EIGENVALUES | MFH_MEASURE_EIGENVECTORS");
    require(!(what & MFH_MEASURE_VON_MISES) || vm, MFH_ERR_INVALID, "the von Mises output was requested but its pointer is null");
    require(!(what & MFH_MEASURE_EIGENVALUES) || eval, MFH_ERR_INVALID, "the eigenvalues were requested but their pointer is null");
    require(!(what & MFH_MEASURE_EIGENVECTORS) || evec, MFH_ERR_INVALID, "the eigenvectors were requested but their pointer is null");
}
// the preconditions of mfh_strain_field
void require_strain_context(mfh_ctx *c) {
    require(c->op == MFH_OP_ELASTICITY, MFH_ERR_STATE, "strain / stress fields are defined for the elasticity operator");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
}
void vertex_average_device(mfh_ctx *c, const double *dField, int nq, int nComp, double *dOut) {
    const HostMesh &m = c->mesh;
    ensure_node_pairs(c);
    k::launch_vertex_average(m.dim, m.npe, m.nVert, c->dNodePtr.p, c->dNodePair.p, c->dGeo.p, c->geoStride, dField, nq, nComp, dOut, c->stream);
}
void require_vertex_average_context(mfh_ctx *c) {
    require(c->mesh.nOwned == c->mesh.nNode, MFH_ERR_UNSUPPORTED,
            "vertex averages need all rows owned: the elements of other ranks are missing at the interface vertices of a row-partitioned context");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
}
} // namespace

mfh_status mfh_sym_measures(mfh_ctx *c, int32_t dim, int64_t n, const double *field, int32_t what, double *vonMises, double *eigenvalues,
                            double *eigenvectors, int32_t onDevice) {
    MFH_TRY(c)
    require(c && field && n >= 0 && (dim == 2 || dim == 3), MFH_ERR_INVALID, "bad arguments");
    require_measure_outputs(what, vonMises, eigenvalues, eigenvectors);
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    const size_t N = (size_t)n, d = (size_t)dim;
    DevInput in(field, N * flat_len(dim), onDevice != 0, c->stream);
    DevOutput vm(vonMises, N, what & MFH_MEASURE_VON_MISES, onDevice != 0), ev(eigenvalues, N * d, what & MFH_MEASURE_EIGENVALUES, onDevice != 0),
        vec(eigenvectors, N * d * d, what & MFH_MEASURE_EIGENVECTORS, onDevice != 0);
    k::launch_sym_measures(dim, n, in.p, what, vm.p, ev.p, vec.p, c->stream);
    vm.finish(c->stream); ev.finish(c->stream); vec.finish(c->stream);
    MFH_HIP(hipStreamSynchronize(c->stream));
    MFH_CATCH(c)
}

mfh_status mfh_stress_measures(mfh_ctx *c, const double *uNodes, int32_t wantStress, int32_t what, double *vonMises, double *eigenvalues,
                               double *eigenvectors, int32_t onDevice) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes, MFH_ERR_STATE, "no mesh set");
    require_measure_outputs(what, vonMises, eigenvalues, eigenvectors);
    require_strain_context(c);
    const HostMesh &m = c->mesh;
    const size_t d = (size_t)m.dim, N = (size_t)m.nElem * (m.deg == 1 ? 1 : d + 1);
    DevInput u(uNodes, (size_t)m.nNode * d, onDevice != 0, c->stream);
    DevOutput vm(vonMises, N, what & MFH_MEASURE_VON_MISES, onDevice != 0), ev(eigenvalues, N * d, what & MFH_MEASURE_EIGENVALUES, onDevice != 0),
        vec(eigenvectors, N * d * d, what & MFH_MEASURE_EIGENVECTORS, onDevice != 0);
    k::launch_stress_measures(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), u.p, wantStress, what, vm.p, ev.p, vec.p, c->stream);
    vm.finish(c->stream); ev.finish(c->stream); vec.finish(c->stream);
    MFH_HIP(hipStreamSynchronize(c->stream));
    MFH_CATCH(c)
}

mfh_status mfh_vertex_average(mfh_ctx *c, const double *field, int32_t perCorner, int32_t nComp, double *out, int32_t onDevice) {
    MFH_TRY(c)
    require(c && c->haveMesh, MFH_ERR_STATE, "no mesh set");
    require(field && out && nComp >= 1, MFH_ERR_INVALID, "bad arguments");
    require_vertex_average_context(c);
    const HostMesh &m = c->mesh;
    const int nq = perCorner ? m.dim + 1 : 1;
    DevInput in(field, (size_t)m.nElem * nq * nComp, onDevice != 0, c->stream);
    DevOutput res(out, (size_t)m.nVert * nComp, true, onDevice != 0);
    vertex_average_device(c, in.p, nq, nComp, res.p);
    res.finish(c->stream);
    MFH_HIP(hipStreamSynchronize(c->stream));
    MFH_CATCH(c)
}

mfh_status mfh_vertex_averaged_strain(mfh_ctx *c, const double *uNodes, int32_t wantStress, double *out, int32_t onDevice) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes && out, MFH_ERR_STATE, "no mesh set");
    require_strain_context(c);
    require_vertex_average_context(c);
    const HostMesh &m = c->mesh;
    const int d = m.dim, fl = flat_len(d), nq = m.deg == 1 ? 1 : d + 1;
    DevInput u(uNodes, (size_t)m.nNode * d, onDevice != 0, c->stream);
    DBuf<double> field;
    field.alloc((size_t)m.nElem * nq * fl);
    k::launch_strain_field(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), u.p, wantStress, field.p, c->stream);
    DevOutput res(out, (size_t)m.nVert * fl, true, onDevice != 0);
    vertex_average_device(c, field.p, nq, fl, res.p);
    res.finish(c->stream);
    MFH_HIP(hipStreamSynchronize(c->stream));
    MFH_CATCH(c)
}

// ---- volume loads: body forces and per-element stress / strain fields (docs/design/04_14_volume_loads.md)
namespace {
void require_volume_load_context(mfh_ctx *c) {
    require(c->mesh.nOwned == c->mesh.nNode, MFH_ERR_UNSUPPORTED,
            "volume loads need all rows owned: the elements of other ranks are missing at the interface nodes of a row-partitioned context");
}
// the load vector as the kernels write it: the caller's device pointer, or a device buffer (holding the caller's values under MFH_LOAD_ADD)
struct LoadOutput {
    DevOutput o;
    LoadOutput(double *dst, size_t n, int32_t flags, hipStream_t s) : o(dst, n, true, (flags & MFH_LOAD_ON_DEVICE) != 0) {
        if (o.host && (flags & MFH_LOAD_ADD) && n) MFH_HIP(hipMemcpyAsync(o.p, dst, n * sizeof(double), hipMemcpyHostToDevice, s));
    }
};
void require_density(mfh_ctx *c, const double *density, bool onDevice) {
    if (!density) return;
    const int64_t n = c->mesh.nElem;
    bool bad = false;
    if (!onDevice) {
        for (int64_t e = 0; e < n && !bad; ++e) bad = !(density[e] >= 0.0) || !std::isfinite(density[e]);
    } else {
        require_device(c);
        MFH_HIP(hipSetDevice(c->device));
        DBuf<int> flag;
        flag.alloc(1);
        flag.zero(c->stream);
        k::launch_density_check(n, density, flag.p, c->stream);
        int h = 0;
        flag.download(&h, 1, c->stream);
        bad = h != 0;
    }
    require(!bad, MFH_ERR_INVALID, "density: an entry is negative or not finite");
}
} // namespace

mfh_status mfh_body_force_load(mfh_ctx *c, int32_t kind, const double *b, const double *density, int32_t flags, double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && !c->external, MFH_ERR_STATE, "no mesh set");
    require_volume_load_context(c);
    require(kind == MFH_BODY_CONSTANT || kind == MFH_BODY_ELEMENT || kind == MFH_BODY_NODE, MFH_ERR_INVALID, "kind: MFH_BODY_CONSTANT | MFH_BODY_ELEMENT | MFH_BODY_NODE");
    require(b && out, MFH_ERR_INVALID, "null argument");
    require((flags & ~(MFH_LOAD_ADD | MFH_LOAD_ON_DEVICE)) == 0, MFH_ERR_INVALID, "flags: MFH_LOAD_ADD | MFH_LOAD_ON_DEVICE");
    const bool onDevice = (flags & MFH_LOAD_ON_DEVICE) != 0;
    require_density(c, density, onDevice);
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
    ensure_dof_pairs(c);
    const HostMesh &m = c->mesh;
    const size_t d = (size_t)m.dim, n = d * (size_t)c->nDoF;
    const size_t nb = kind == MFH_BODY_ELEMENT ? (size_t)m.nElem * d : (kind == MFH_BODY_NODE ? (size_t)m.nNode * d : 0);
    DevInput bIn(kind == MFH_BODY_CONSTANT ? nullptr : b, nb, onDevice, c->stream), rho(density, density ? (size_t)m.nElem : 0, onDevice, c->stream);
    LoadOutput res(out, n, flags, c->stream);
    k::launch_body_force_load(asm_args(c), c->nDoF, dof_pair_ptr(c), dof_pair_list(c), c->tables, kind, c->dElemNodes.p, bIn.p, b, density ? rho.p : nullptr,
                              (flags & MFH_LOAD_ADD) != 0, res.o.p, c->stream);
    res.o.finish(c->stream);
    MFH_HIP(hipStreamSynchronize(c->stream));
    MFH_CATCH(c)
}

mfh_status mfh_stress_field_load(mfh_ctx *c, int32_t kind, const double *field, double *stressOut, int32_t flags, double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && !c->external, MFH_ERR_STATE, "no mesh set");
    require_volume_load_context(c);
    require(c->op == MFH_OP_ELASTICITY, MFH_ERR_UNSUPPORTED, "the stress-field load is defined for the elasticity operator");
    require(kind == MFH_FIELD_LOAD_STRESS || kind == MFH_FIELD_LOAD_STRAIN, MFH_ERR_INVALID, "kind: MFH_FIELD_LOAD_STRESS | MFH_FIELD_LOAD_STRAIN");
    require(field && out, MFH_ERR_INVALID, "null argument");
    require(!(stressOut && kind == MFH_FIELD_LOAD_STRESS), MFH_ERR_INVALID, "stressOut goes with MFH_FIELD_LOAD_STRAIN: a stress field is its own stress");
    require((flags & ~(MFH_LOAD_ADD | MFH_LOAD_ON_DEVICE)) == 0, MFH_ERR_INVALID, "flags: MFH_LOAD_ADD | MFH_LOAD_ON_DEVICE");
    const bool onDevice = (flags & MFH_LOAD_ON_DEVICE) != 0;
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
    ensure_dof_pairs(c);
    const HostMesh &m = c->mesh;
    const size_t nf = (size_t)m.nElem * flat_len(m.dim), n = (size_t)m.dim * (size_t)c->nDoF;
    DevInput in(field, nf, onDevice, c->stream);
    LoadOutput res(out, n, flags, c->stream);
    DevOutput sig(stressOut, nf, stressOut != nullptr, onDevice);
    const k::AsmArgs a = asm_args(c);
    k::launch_stress_field_load(a, c->nDoF, dof_pair_ptr(c), dof_pair_list(c), c->tables, kind == MFH_FIELD_LOAD_STRAIN, in.p, (flags & MFH_LOAD_ADD) != 0,
                                res.o.p, c->stream);
    if (stressOut) k::launch_field_stress(a, in.p, sig.p, c->stream);
    res.o.finish(c->stream);
    sig.finish(c->stream);
    MFH_HIP(hipStreamSynchronize(c->stream));
    MFH_CATCH(c)
}

mfh_status mfh_peak_von_mises(mfh_ctx *c, const double *uNodes, int32_t wantStress, double *value, int64_t *cornerIndex) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes, MFH_ERR_STATE, "no mesh set");
    require(value || cornerIndex, MFH_ERR_INVALID, "null outputs");
    require_strain_context(c);
    const HostMesh &m = c->mesh;
    require(m.nElem > 0, MFH_ERR_INVALID, "the mesh has no elements");
    DevInput u(uNodes, (size_t)m.nNode * m.dim, false, c->stream);
    DBuf<double> partV, outV;
    DBuf<int64_t> partI, outI;
    partV.alloc(k::PEAK_GRID_CAP); partI.alloc(k::PEAK_GRID_CAP);
    outV.alloc(1); outI.alloc(1);
    k::launch_peak_von_mises(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), u.p, wantStress, partV.p, partI.p, outV.p, outI.p, c->stream);
    double v = 0;
    int64_t i = 0;
    outV.download(&v, 1, c->stream);
    outI.download(&i, 1, c->stream);
    if (value) *value = v;
    if (cornerIndex) *cornerIndex = i;
    MFH_CATCH(c)
}

mfh_status mfh_mutual_energy_differential(mfh_ctx *c, const double *w, double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && w && out, MFH_ERR_STATE, "no mesh set");
    require(c->op == MFH_OP_ELASTICITY, MFH_ERR_STATE, "mutual energies are defined for the elasticity operator");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
    const HostMesh &m = c->mesh;
    const int d = m.dim, fl = flat_len(d), np = fl * (fl + 1) / 2;
    DBuf<double> wd, res;
    wd.alloc((size_t)fl * m.nNode * d);
    MFH_HIP(hipMemcpyAsync(wd.p, w, wd.n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    res.alloc((size_t)np * m.nVert * d);
    res.zero(c->stream);
    k::launch_mutual_energy_differential(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), wd.p, m.nNode, m.nVert, res.p, c->stream);
    res.download(out, res.n, c->stream);
    MFH_CATCH(c)
}

static void average_strain_impl(mfh_ctx *c, const double *uNodes, double *out, bool stress, const double *uFixed = nullptr,
                                const double *deltaP = nullptr) {
    require(c->op == MFH_OP_ELASTICITY, MFH_ERR_STATE, "strain / stress fields are defined for the elasticity operator");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
    const HostMesh &m = c->mesh;
    const int d = m.dim, fl = flat_len(d);
    c->wx.alloc((size_t)m.nNode * d);
    MFH_HIP(hipMemcpyAsync(c->wx.p, uNodes, (size_t)m.nNode * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    DBuf<double> res, dp, uf;
    if (deltaP) {
        upload_delta_p(c, deltaP, dp);
        uf.alloc((size_t)m.nNode * d);
        MFH_HIP(hipMemcpyAsync(uf.p, uFixed, (size_t)m.nNode * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    res.alloc((size_t)m.nElem * fl);
    k::launch_average_strain(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), c->wx.p, res.p, stress ? 1 : 0,
                             deltaP ? uf.p : nullptr, deltaP ? dp.p : nullptr, c->stream);
    res.download(out, res.n, c->stream);
}

mfh_status mfh_delta_average_strain(mfh_ctx *c, const double *uNodes, const double *deltaU, const double *deltaP, int32_t wantStress,
                                    double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes && deltaU && deltaP && out, MFH_ERR_STATE, "no mesh set");
    average_strain_impl(c, deltaU, out, wantStress != 0, uNodes, deltaP);
    MFH_CATCH(c)
}

mfh_status mfh_set_operator(mfh_ctx *c, int32_t op) {
    MFH_TRY(c)
    require(c && (op == MFH_OP_ELASTICITY || op == MFH_OP_LAPLACIAN || op == MFH_OP_MASS || op == MFH_OP_MASS_VECTOR), MFH_ERR_INVALID, "unknown operator");
    require(!(op == MFH_OP_ELASTICITY && c->opDegree == 1 && c->haveMesh && c->mesh.deg == 2), MFH_ERR_STATE,
            "forced degree 1 is defined for the Laplacian and mass operators: call mfh_set_operator_degree(ctx, 0) before selecting elasticity");
    require(!(op == MFH_OP_MASS_VECTOR && dist_active(c)), MFH_ERR_UNSUPPORTED, "the vector-valued mass operator (MFH_OP_MASS_VECTOR) is not available on row-partitioned contexts");
    if (c->p1) {                       // the forced-degree-1 view carries the same operator (elasticity excepted: it has none)
        const mfh_status st = op == MFH_OP_ELASTICITY ? MFH_OK : mfh_set_operator(c->p1, op);
        if (st != MFH_OK) throw Error(st, c->p1->err);
    }
    if (op != c->op) {
        c->op = op;
        invalidate_matrix(c);          // pattern and gather lists are shared by all operators; only the values change
        refresh_storage_rule(c);       // ... unless the storage of K follows the operator (quadratic elasticity: upper triangle)
        if (c->haveMesh) clear_fixed(c);   // the variable numbering changes with the block size
    }
    MFH_CATCH(c)
}

mfh_status mfh_average_gradient(mfh_ctx *c, const double *uNodes, double *grad) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes && grad, MFH_ERR_STATE, "no mesh set");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
    const HostMesh &m = c->mesh;
    c->wx.alloc((size_t)m.nNode);
    MFH_HIP(hipMemcpyAsync(c->wx.p, uNodes, (size_t)m.nNode * sizeof(double), hipMemcpyHostToDevice, c->stream));
    DBuf<double> res;
    res.alloc((size_t)m.nElem * m.dim);
    k::launch_average_gradient(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), c->wx.p, res.p, c->stream);
    res.download(grad, res.n, c->stream);
    MFH_CATCH(c)
}

mfh_status mfh_matrix_free_info(mfh_ctx *c, int32_t *active, int32_t *mode, int64_t *nBlocks, int64_t *nBlockRows, int64_t *nInterface,
                                int32_t *maxBlockRows) {
    MFH_TRY(c)
    require(c && c->haveMesh, MFH_ERR_STATE, "no mesh set");
    if (active) *active = c->use_mf() ? 1 : 0;
    if (c->use_mf() && c->mfModeEff() == 4 && c->op == MFH_OP_ELASTICITY) {
        require_device(c);
        MFH_HIP(hipSetDevice(c->device));
        ensure_mf_cluster(c);
    }
    if (mode) *mode = c->mfModeEff();
    if (nBlocks) *nBlocks = c->mfcValid ? c->mfc.nBlocks : 0;
    if (nBlockRows) *nBlockRows = c->mfcValid ? c->mfc.nEntries : 0;
    if (nInterface) *nInterface = c->mfcValid ? c->mfc.nIface : 0;
    if (maxBlockRows) *maxBlockRows = c->mfcValid ? c->mfc.maxLocal : 0;
    MFH_CATCH(c)
}

mfh_status mfh_average_strain(mfh_ctx *c, const double *uNodes, double *strain) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes && strain, MFH_ERR_STATE, "no mesh set");
    average_strain_impl(c, uNodes, strain, false);
    MFH_CATCH(c)
}
mfh_status mfh_average_stress(mfh_ctx *c, const double *uNodes, double *stress) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes && stress, MFH_ERR_STATE, "no mesh set");
    average_strain_impl(c, uNodes, stress, true);
    MFH_CATCH(c)
}
// sum_e vol_e C_e : (average strain_e(u) + cstrain): the element loop of homogenizedElasticityTensor reduced on the device
mfh_status mfh_integrated_stress(mfh_ctx *c, const double *uNodes, const double *cstrainFlat, double *out) {
    MFH_TRY(c)
    require(c && c->haveMesh && uNodes && out, MFH_ERR_STATE, "no mesh set");
    require(c->op == MFH_OP_ELASTICITY, MFH_ERR_STATE, "strain / stress fields are defined for the elasticity operator");
    require_device(c);
    MFH_HIP(hipSetDevice(c->device));
    ensure_geometry(c);
    const HostMesh &m = c->mesh;
    const int d = m.dim, fl = flat_len(d);
    c->wx.alloc((size_t)m.nNode * d);
    MFH_HIP(hipMemcpyAsync(c->wx.p, uNodes, (size_t)m.nNode * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    DBuf<double> acc;
    acc.alloc((size_t)fl);
    acc.zero(c->stream);
    k::launch_average_strain(asm_args(c), c->dElemNodes.p, c->tables.intGrad.data(), c->wx.p, nullptr, 1, nullptr, nullptr, c->stream, cstrainFlat, acc.p);
    acc.download(out, (size_t)fl, c->stream);
    MFH_CATCH(c)
}

} // extern "C"
