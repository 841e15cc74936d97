// Differential operators of a FEM mesh on the MI355X path: the facade of the reference's Laplacian.hh / MassMatrix.hh over the C ABI
// (include/meshfem_hip.h).
//   Laplacian::construct<Deg>(simOrCtx)                        == Laplacian::construct<Deg>(mesh)                 (Laplacian.hh:97-104)
//   MassMatrix::construct<Deg>(simOrCtx, lumped)               == MassMatrix::construct<Deg>(mesh, lumped)        (MassMatrix.hh:102-129)
//   MassMatrix::construct_vector_valued<Deg>(simOrCtx, lumped) == MassMatrix::construct_vector_valued<Deg>(...)   (MassMatrix.hh:131-147)
// Deg is deduced from the mesh unless given; Deg = 1 on a quadratic mesh is the forced-degree-1 view of the same context
// (mfh_set_operator_degree: no second mesh). The result is the upper triangle after sumRepeated, in column-major order. The argument is a
// Simulator (anything with ctx(); it is handed back with the elasticity operator selected) or a raw mfh_ctx* with a mesh (handed back with
// the operator that was assembled and the full degree).
#pragma once

#include <limits>

#include "LinearElasticity.hh"

namespace MeshFEMHip {
namespace detail {

constexpr size_t kMeshDegree = std::numeric_limits<size_t>::max();

inline int64_t meshVertexCount(mfh_ctx *c) {
    int64_t nVert = 0;
    check(c, mfh_mesh_sizes(c, nullptr, nullptr, &nVert, nullptr, nullptr, nullptr, nullptr));
    return nVert;
}

// upper triplets (or the lumped diagonal) of `op` at the degree asked for; the context leaves with the full degree in force
template <size_t Deg> TripletMatrix operatorTriplets(mfh_ctx *c, int32_t op, bool lumped) {
    static_assert(Deg == kMeshDegree || Deg == 1 || Deg == 2, "degree must be 1, 2 or deduced");
    check(c, mfh_set_operator_degree(c, 0));
    check(c, mfh_set_operator(c, op));
    check(c, mfh_set_operator_degree(c, Deg == 1 ? 1 : 0));
    struct Restore { mfh_ctx *c; ~Restore() { mfh_set_operator_degree(c, 0); } } restore{c};
    check(c, mfh_assemble(c, MFH_ASSEMBLE_GATHER));
    int64_t nRows = 0;
    check(c, mfh_matrix_info(c, &nRows, nullptr, nullptr));
    if (Deg == 2 && nRows == meshVertexCount(c)) throw std::runtime_error("Degree 2 operators need a quadratic mesh");
    int64_t nElem = 0;
    int32_t npe = 0;
    check(c, mfh_mesh_sizes(c, &nElem, nullptr, nullptr, nullptr, nullptr, &npe, nullptr));
    const size_t dim = npe == 3 || npe == 6 ? 2 : 3;
    const size_t n = (size_t)nRows * (op == MFH_OP_MASS_VECTOR ? dim : 1);
    TripletMatrix T;
    T.m = T.n = n;
    if (lumped) {
        std::vector<Real> d(n);
        check(c, mfh_mass_lumped(c, d.data(), 0));
        T.nz.resize(n);
        for (size_t k = 0; k < n; ++k) T.nz[k] = Triplet{k, k, d[k]};
        return T;
    }
    uint64_t cap = 0;
    check(c, mfh_export_upper_triplets(c, nullptr, nullptr, nullptr, &cap));
    std::vector<uint64_t> i(cap), j(cap);
    std::vector<Real> v(cap);
    check(c, mfh_export_upper_triplets(c, i.data(), j.data(), v.data(), &cap));
    T.nz.resize(cap);
    for (uint64_t k = 0; k < cap; ++k) T.nz[k] = Triplet{(size_t)i[k], (size_t)j[k], v[k]};
    return T;
}

// a Simulator goes back to the elasticity operator
template <class Sim> struct SimulatorGuard {
    mfh_ctx *c;
    ~SimulatorGuard() { mfh_set_operator_degree(c, 0); mfh_set_operator(c, MFH_OP_ELASTICITY); }
};

}   // namespace detail

namespace Laplacian {
template <size_t Deg = detail::kMeshDegree> TripletMatrix construct(mfh_ctx *ctx) { return detail::operatorTriplets<Deg>(ctx, MFH_OP_LAPLACIAN, false); }
template <size_t Deg = detail::kMeshDegree, class Sim> auto construct(const Sim &sim) -> decltype(sim.ctx(), TripletMatrix()) {
    detail::SimulatorGuard<Sim> g{sim.ctx()};
    return detail::operatorTriplets<Deg>(sim.ctx(), MFH_OP_LAPLACIAN, false);
}
}   // namespace Laplacian

namespace MassMatrix {
template <size_t Deg = detail::kMeshDegree> TripletMatrix construct(mfh_ctx *ctx, bool lumped = false) { return detail::operatorTriplets<Deg>(ctx, MFH_OP_MASS, lumped); }
template <size_t Deg = detail::kMeshDegree, class Sim> auto construct(const Sim &sim, bool lumped = false) -> decltype(sim.ctx(), TripletMatrix()) {
    detail::SimulatorGuard<Sim> g{sim.ctx()};
    return detail::operatorTriplets<Deg>(sim.ctx(), MFH_OP_MASS, lumped);
}
template <size_t Deg = detail::kMeshDegree> TripletMatrix construct_vector_valued(mfh_ctx *ctx, bool lumped = false) {
    return detail::operatorTriplets<Deg>(ctx, MFH_OP_MASS_VECTOR, lumped);
}
template <size_t Deg = detail::kMeshDegree, class Sim> auto construct_vector_valued(const Sim &sim, bool lumped = false) -> decltype(sim.ctx(), TripletMatrix()) {
    detail::SimulatorGuard<Sim> g{sim.ctx()};
    return detail::operatorTriplets<Deg>(sim.ctx(), MFH_OP_MASS_VECTOR, lumped);
}
}   // namespace MassMatrix

}   // namespace MeshFEMHip
