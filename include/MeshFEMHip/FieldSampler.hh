// Point queries on a mesh on the MI355X path: the facade of the reference's FieldSampler.hh over the C ABI (include/meshfem_hip.h, "field
// sampler on the device"; docs/design/04_11_field_sampler.md).
//   FieldSampler fs(sim);            over a Simulator (anything with ctx()), or over a raw mfh_ctx* that holds a mesh; neither is owned
//   FieldSampler fs(dim, V, F);      a raw mesh (flat vertex coordinates and element corners): a degree-1 context of its own
//   fs.closestElementAndPoint(P, I, C)          element and closest point of the mesh per query point (C = P inside the mesh)
//   fs.closestElementAndBaryCoords(P, I, B)     element and barycentric coordinates of that point
//   fs.closestNodeAndSqDist(P, NI, sqDist)      node with the largest shape function there; "Unsupported for raw meshes" like the reference
//   fs.contains(P, eps = 1e-10)                 squared distance to the mesh <= eps^2
//   fs.sample(P, fieldValues, rows)             per-vertex, per-element or per-node field (detected from `rows` in that order) at the points
// Points and fields are flat row-major arrays: P holds nP x dim numbers. Differences from the reference: a uniform cell grid instead of the
// AABB tree; a point shared by several elements goes to the one with the LOWEST index.
#pragma once

#include "LinearElasticity.hh"

#include <memory>

namespace MeshFEMHip {

class FieldSampler {
public:
    template <class Sim> explicit FieldSampler(const Sim &sim) : m_ctx(sim.ctx()) { readSizes(); }
    explicit FieldSampler(mfh_ctx *ctx) : m_ctx(ctx) { readSizes(); }
    FieldSampler(int dim, const std::vector<Real> &V, const std::vector<int32_t> &F, int device = 0) : m_own(new Context(device)), m_raw(true) {
        m_ctx = m_own->get();
        if ((dim != 2 && dim != 3) || V.size() % (size_t)dim || F.size() % (size_t)(dim + 1)) throw std::runtime_error("FieldSampler: V must be nVert x dim and F nElem x (dim + 1)");
        check(m_ctx, mfh_mesh_build(m_ctx, dim, 1, (int64_t)(F.size() / (size_t)(dim + 1)), (int64_t)(V.size() / (size_t)dim), F.data(), V.data()));
        readSizes();
    }

    size_t dim() const { return m_dim; }
    mfh_ctx *ctx() const { return m_ctx; }

    void closestElementAndPoint(const std::vector<Real> &P, std::vector<int32_t> &I, std::vector<Real> &C) const {
        std::vector<Real> sqDist;
        closestElementAndPoint(P, sqDist, I, C);
    }
    void closestElementAndPoint(const std::vector<Real> &P, std::vector<Real> &sqDist, std::vector<int32_t> &I, std::vector<Real> &C) const {
        const size_t n = numPoints(P);
        I.resize(n); C.resize(n * m_dim); sqDist.resize(n);
        check(m_ctx, mfh_locate(m_ctx, (int64_t)n, P.data(), I.data(), nullptr, C.data(), sqDist.data(), 0));
    }
    void closestElementAndBaryCoords(const std::vector<Real> &P, std::vector<int32_t> &I, std::vector<Real> &B) const {
        const size_t n = numPoints(P);
        I.resize(n); B.resize(n * (m_dim + 1));
        check(m_ctx, mfh_locate(m_ctx, (int64_t)n, P.data(), I.data(), B.data(), nullptr, nullptr, 0));
    }
    void closestNodeAndSqDist(const std::vector<Real> &P, std::vector<int32_t> &NI, std::vector<Real> &sqDist) const {
        if (m_raw) throw std::runtime_error("Unsupported for raw meshes");
        const size_t n = numPoints(P);
        NI.resize(n); sqDist.resize(n);
        check(m_ctx, mfh_closest_node(m_ctx, (int64_t)n, P.data(), NI.data(), sqDist.data(), 0));
    }
    std::vector<bool> contains(const std::vector<Real> &P, Real eps = 1e-10) const {
        const size_t n = numPoints(P);
        std::vector<Real> sqDist(n);
        check(m_ctx, mfh_locate(m_ctx, (int64_t)n, P.data(), nullptr, nullptr, nullptr, sqDist.data(), 0));
        std::vector<bool> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = sqDist[i] <= eps * eps;
        return out;
    }
    // fieldValues: rows x nComp, row-major; returns nP x nComp
    std::vector<Real> sample(const std::vector<Real> &P, const std::vector<Real> &fieldValues, size_t rows) const {
        const size_t n = numPoints(P);
        int32_t kind;
        if (rows == m_nVert) kind = MFH_FIELD_PER_VERTEX;
        else if (rows == m_nElem) kind = MFH_FIELD_PER_ELEMENT;
        else if (rows == m_nNode) kind = MFH_FIELD_PER_NODE;
        else throw std::runtime_error("Invalid fieldValues size");
        if (rows == 0 || fieldValues.size() % rows || fieldValues.empty()) throw std::runtime_error("Invalid fieldValues size");
        const size_t nComp = fieldValues.size() / rows;
        std::vector<Real> out(n * nComp);
        check(m_ctx, mfh_sample_field(m_ctx, (int64_t)n, P.data(), kind, fieldValues.data(), (int32_t)nComp, out.data(), 0));
        return out;
    }

private:
    size_t numPoints(const std::vector<Real> &P) const {
        if (P.size() % m_dim) throw std::runtime_error("FieldSampler: P must hold nP x dim numbers");
        return P.size() / m_dim;
    }
    void readSizes() {
        int64_t ne = 0, nn = 0, nv = 0;
        int32_t npe = 0;
        check(m_ctx, mfh_mesh_sizes(m_ctx, &ne, &nn, &nv, nullptr, nullptr, &npe, nullptr));
        m_nElem = (size_t)ne; m_nNode = (size_t)nn; m_nVert = (size_t)nv;
        m_dim = (npe == 3 || npe == 6) ? 2 : 3;
    }
    std::unique_ptr<Context> m_own;
    mfh_ctx *m_ctx = nullptr;
    bool m_raw = false;
    size_t m_dim = 0, m_nElem = 0, m_nNode = 0, m_nVert = 0;
};

} // namespace MeshFEMHip
