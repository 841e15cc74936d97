// Field post-processing on the MI355X path: the facade of the reference's FieldPostProcessing.hh over the C ABI (include/meshfem_hip.h).
//   vertexAveragedField(sim, cornerValues)   == vertexAveragedField(mesh, f) (FieldPostProcessing.hh:24-47): the C0 volume-weighted average of
//                                            the element corner values meeting at every vertex. The reference takes f(element, barycentric
//                                            point) and evaluates it at the corners; here the corner values themselves are passed:
//                                            numElements() x (N+1) entries, element-major, or numElements() entries for a per-element constant.
//                                            Entries are Real or std::array<Real, C> (vector, flattened symmetric, full tensor); the result
//                                            has one entry per mesh vertex.
//   vertexAveragedStress / vertexAveragedStrain(sim, uNodes)   the average of Simulator::stressField / strainField with the corner field
//                                            kept on the device; [nVert] flattened symmetric matrices
// sim: a Simulator (anything with ctx() and numElements()). Row-partitioned contexts are refused (std::runtime_error).
#pragma once

#include "LinearElasticity.hh"

namespace MeshFEMHip {
namespace detail {

template <class Sim> void vertexAverage(const Sim &sim, const Real *field, size_t nEntries, size_t nComp, std::vector<Real> &flatOut, size_t &nVert) {
    int64_t nv = 0;
    int32_t npe = 0;
    check(sim.ctx(), mfh_mesh_sizes(sim.ctx(), nullptr, nullptr, &nv, nullptr, nullptr, &npe, nullptr));
    const size_t nElem = sim.numElements(), corners = npe == 3 || npe == 6 ? 3 : 4;
    if (nEntries != nElem && nEntries != nElem * corners) throw std::runtime_error("vertexAveragedField: one value per element or per element corner expected");
    nVert = (size_t)nv;
    flatOut.resize(nVert * nComp);
    check(sim.ctx(), mfh_vertex_average(sim.ctx(), field, nEntries == nElem ? 0 : 1, (int32_t)nComp, flatOut.data(), 0));
}

} // namespace detail

template <class Sim, size_t C>
std::vector<std::array<Real, C>> vertexAveragedField(const Sim &sim, const std::vector<std::array<Real, C>> &cornerValues) {
    size_t nVert = 0;
    std::vector<Real> flat;
    detail::vertexAverage(sim, cornerValues.empty() ? nullptr : &cornerValues[0][0], cornerValues.size(), C, flat, nVert);
    std::vector<std::array<Real, C>> out(nVert);
    for (size_t v = 0; v < nVert; ++v)
        for (size_t c = 0; c < C; ++c) out[v][c] = flat[v * C + c];
    return out;
}

template <class Sim> std::vector<Real> vertexAveragedField(const Sim &sim, const std::vector<Real> &cornerValues) {
    size_t nVert = 0;
    std::vector<Real> out;
    detail::vertexAverage(sim, cornerValues.data(), cornerValues.size(), 1, out, nVert);
    return out;
}

template <class Sim> typename Sim::SMField vertexAveragedStrain(const Sim &sim, const typename Sim::VField &uNodes, bool stress = false) {
    int64_t nv = 0;
    check(sim.ctx(), mfh_mesh_sizes(sim.ctx(), nullptr, nullptr, &nv, nullptr, nullptr, nullptr, nullptr));
    typename Sim::SMField out((size_t)nv);
    check(sim.ctx(), mfh_vertex_averaged_strain(sim.ctx(), &uNodes[0][0], stress ? 1 : 0, &out[0][0], 0));
    return out;
}
template <class Sim> typename Sim::SMField vertexAveragedStress(const Sim &sim, const typename Sim::VField &uNodes) {
    return vertexAveragedStrain(sim, uNodes, true);
}

} // namespace MeshFEMHip
