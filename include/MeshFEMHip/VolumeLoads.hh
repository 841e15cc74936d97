// Volume loads on the MI355X path: body forces and thermal strain over the C ABI (include/meshfem_hip.h, "volume loads"; docs/design/04_14_volume_loads.md).
// The reference's interior load is Simulator::perElementStressFieldLoad (LinearElasticity.hh:564-577), a member of the Simulator here as there; it has
// no body force and no thermal load, so the functions of this file have no counterpart to cite. Free functions on a Simulator, like Dynamics.hh:
//   bodyForceLoad(sim, b, density)        f_i = sum_e density_e int_e phi_i b; b one vector, one per element (constant on it) or one per node
//                                         (interpolated with the mesh's shape functions); density per element or empty (= 1)
//   gravityLoad(sim, g, density)          the load of density x g, density one number for the whole body
//   thermalLoad(sim, alpha, dT)           the load of the thermal strain eps_th = alpha_e dT_e I (one value per element each)
//   thermalStress(sim, u, alpha, dT)      stressField(u) - C : eps_th in stressField's layout [nElem][1 | N+1][flatLen]
// Every load is a per-DoF field that solve, solveMany and transient take as it stands. The device gathers per DoF in a fixed order without atomics:
// the same call returns the same bits. Throws std::runtime_error where the C call fails.
#pragma once

#include "LinearElasticity.hh"

namespace MeshFEMHip {

template <class Sim>
typename Sim::VField bodyForceLoad(const Sim &sim, const typename Sim::VField &b, const std::vector<Real> &density = std::vector<Real>()) {
    const size_t nE = sim.numElements(), nN = sim.numNodes();
    if (!density.empty() && density.size() != nE) throw std::runtime_error("bodyForceLoad: one density per element expected");
    const bool one = b.size() == 1, elem = b.size() == nE, node = b.size() == nN;
    if (!one && elem == node) throw std::runtime_error(elem ? "bodyForceLoad: as many elements as nodes, the kind of b is ambiguous (call mfh_body_force_load)"
                                                            : "bodyForceLoad: b needs 1, numElements() or numNodes() vectors");
    typename Sim::VField f(sim.numDoFs());
    check(sim.ctx(), mfh_body_force_load(sim.ctx(), one ? MFH_BODY_CONSTANT : (elem ? MFH_BODY_ELEMENT : MFH_BODY_NODE), &b[0][0],
                                         density.empty() ? nullptr : density.data(), 0, &f[0][0]));
    return f;
}

template <class Sim>
typename Sim::VField gravityLoad(const Sim &sim, const typename Sim::VField::value_type &g, Real density = 1.0) {
    return bodyForceLoad(sim, typename Sim::VField(1, g), std::vector<Real>(sim.numElements(), density));
}

template <class Sim>
typename Sim::SMField thermalStrain(const Sim &sim, const std::vector<Real> &alpha, const std::vector<Real> &dT) {
    constexpr size_t N = std::tuple_size<typename Sim::VField::value_type>::value;
    if (alpha.size() != sim.numElements() || dT.size() != sim.numElements()) throw std::runtime_error("thermal strain: one alpha and one dT per element expected");
    typename Sim::SMField eps(sim.numElements());
    for (size_t e = 0; e < eps.size(); ++e) {
        eps[e].fill(0.0);
        for (size_t a = 0; a < N; ++a) eps[e][a] = alpha[e] * dT[e];
    }
    return eps;
}

template <class Sim>
typename Sim::VField thermalLoad(const Sim &sim, const std::vector<Real> &alpha, const std::vector<Real> &dT) {
    return sim.perElementStressFieldLoad(thermalStrain(sim, alpha, dT), true);
}

template <class Sim>
std::vector<Real> thermalStress(const Sim &sim, const typename Sim::VField &uNodes, const std::vector<Real> &alpha, const std::vector<Real> &dT) {
    const typename Sim::SMField eps = thermalStrain(sim, alpha, dT);
    typename Sim::SMField sig(eps.size());
    typename Sim::VField f(sim.numDoFs());
    check(sim.ctx(), mfh_stress_field_load(sim.ctx(), MFH_FIELD_LOAD_STRAIN, &eps[0][0], &sig[0][0], 0, &f[0][0]));
    std::vector<Real> s = sim.stressField(uNodes);
    constexpr size_t FL = std::tuple_size<typename Sim::SMField::value_type>::value;
    const size_t nq = s.size() / (sig.size() * FL);
    for (size_t e = 0; e < sig.size(); ++e)
        for (size_t q = 0; q < nq; ++q)
            for (size_t k = 0; k < FL; ++k) s[(e * nq + q) * FL + k] -= sig[e][k];
    return s;
}

} // namespace MeshFEMHip
