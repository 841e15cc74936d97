// Linear buckling on the MI355X path, over the C ABI (include/meshfem_hip.h, "linear buckling"). The reference has no counterpart: its Eigensolver.hh
// has no buckling entry.
//   setPrestress(sim, sigma)             the prestress field of the geometric stiffness: one flattened symmetric tensor per element (flatLen values,
//                                        tensor shear entries, the layout of the average stress field); an empty vector clears it
//   prestressFromDisplacement(sim, u)    the field becomes C_e : (element-average strain of u), u one N-vector per NODE, on the device
//   applyGeometricStiffness(sim, x)      Kg x for one N-vector per DoF, no variables masked
//   bucklingModes(sim, nev, opt, info)   {load factors (ascending, nev; +infinity where the prestress does not buckle the body), shapes (nev fields of
//                                        one N-vector per DoF, K-orthonormal, largest entry positive)} of (K + factor Kg) x = 0; the Dirichlet variables
//                                        of the boundary conditions applied to the Simulator are the clamp and must leave no rigid motion free
//   prestressedModes(sim, nev, s, ...)   {lambda (ascending, nev; negative beyond the critical load), shapes (M-orthonormal)} of
//                                        (K + s Kg) x = lambda density M x: the vibrational modes of Eigensolver.hh under s times the prestress;
//                                        start (may be empty): the shapes of a neighbouring load factor to start from
//   applyTangentStiffness(sim, s, x)     (K + s Kg) x for one N-vector per DoF, no variables masked
// LOBPCG on the device with the Simulator's preconditioner; each throws std::runtime_error where the C call fails, a tolerance that maxit iterations
// do not reach included.
#pragma once

#include <utility>

#include "Eigensolver.hh"
#include "LinearElasticity.hh"

namespace MeshFEMHip {

struct BucklingOptions {
    Real rtol = 1e-6;       // ||Kg x - mu K x|| / (|mu| ||K x||) per mode
    int maxit = 500;
};

template <class Sim>
void setPrestress(const Sim &sim, const std::vector<Real> &sigma) {
    constexpr size_t N = std::tuple_size<typename Sim::VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    if (sigma.size() % (N * (N + 1) / 2) != 0) throw std::runtime_error("setPrestress: flatLen values per element");
    check(c, mfh_set_prestress(c, sigma.empty() ? nullptr : sigma.data(), (int64_t)(sigma.size() / (N * (N + 1) / 2)), 0));
}

template <class Sim>
void prestressFromDisplacement(const Sim &sim, const typename Sim::VField &uNodes) {
    mfh_ctx *c = sim.ctx();
    int64_t nNode = 0;
    check(c, mfh_mesh_sizes(c, nullptr, &nNode, nullptr, nullptr, nullptr, nullptr, nullptr));
    if ((int64_t)uNodes.size() != nNode) throw std::runtime_error("prestressFromDisplacement: u needs one entry per node");
    check(c, mfh_prestress_from_displacement(c, &uNodes[0][0], 0));
}

template <class Sim>
typename Sim::VField applyGeometricStiffness(const Sim &sim, const typename Sim::VField &x) {
    mfh_ctx *c = sim.ctx();
    if (x.size() != sim.numDoFs()) throw std::runtime_error("applyGeometricStiffness: x needs one entry per DoF");
    typename Sim::VField y(x.size());
    check(c, mfh_geometric_apply(c, &x[0][0], &y[0][0], 0));
    return y;
}

template <class Sim>
std::pair<std::vector<Real>, std::vector<typename Sim::VField>> bucklingModes(const Sim &sim, int nev, const BucklingOptions &opt = BucklingOptions(),
                                                                              mfh_buckling_info *info = nullptr) {
    constexpr size_t N = std::tuple_size<typename Sim::VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    check(c, mfh_clear_fixed(c));
    int64_t nv = 0;
    check(c, mfh_bc_dirichlet_vars(c, nullptr, nullptr, &nv));
    std::vector<int64_t> vars((size_t)nv);
    std::vector<Real> vals((size_t)nv);
    if (nv > 0) {
        check(c, mfh_bc_dirichlet_vars(c, vars.data(), vals.data(), &nv));
        check(c, mfh_fix_variables(c, nv, vars.data(), nullptr));
    }
    const size_t nDoF = sim.numDoFs(), k = nev > 0 ? (size_t)nev : 0;
    std::vector<Real> factors(k), flat(k * nDoF * N);
    check(c, mfh_buckling(c, nev, 0, opt.rtol, opt.maxit, factors.data(), flat.data(), nullptr, info));
    std::vector<typename Sim::VField> modes(k, typename Sim::VField(nDoF));
    for (size_t m = 0; m < k; ++m)
        for (size_t i = 0; i < nDoF; ++i)
            for (size_t a = 0; a < N; ++a) modes[m][i][a] = flat[(m * nDoF + i) * N + a];
    return {factors, modes};
}

template <class Sim>
typename Sim::VField applyTangentStiffness(const Sim &sim, Real loadFactor, const typename Sim::VField &x) {
    mfh_ctx *c = sim.ctx();
    if (x.size() != sim.numDoFs()) throw std::runtime_error("applyTangentStiffness: x needs one entry per DoF");
    typename Sim::VField y(x.size());
    check(c, mfh_tangent_apply(c, loadFactor, &x[0][0], &y[0][0], 0));
    return y;
}

template <class Sim>
std::pair<std::vector<Real>, std::vector<typename Sim::VField>> prestressedModes(const Sim &sim, int nev, Real loadFactor, Real density = 1.0,
                                                                                 const ModesOptions &opt = ModesOptions(), mfh_modes_info *info = nullptr,
                                                                                 const std::vector<typename Sim::VField> &start = {}) {
    constexpr size_t N = std::tuple_size<typename Sim::VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    check(c, mfh_clear_fixed(c));
    int64_t nv = 0;
    check(c, mfh_bc_dirichlet_vars(c, nullptr, nullptr, &nv));
    std::vector<int64_t> vars((size_t)nv);
    std::vector<Real> vals((size_t)nv);
    if (nv > 0) {
        check(c, mfh_bc_dirichlet_vars(c, vars.data(), vals.data(), &nv));
        check(c, mfh_fix_variables(c, nv, vars.data(), nullptr));
    }
    const size_t nDoF = sim.numDoFs(), k = nev > 0 ? (size_t)nev : 0;
    std::vector<Real> lambda(k), flat(k * nDoF * N), x0;
    if (!start.empty()) {
        if (start.size() != k) throw std::runtime_error("prestressedModes: start needs nev fields");
        x0.resize(k * nDoF * N);
        for (size_t m = 0; m < k; ++m) {
            if (start[m].size() != nDoF) throw std::runtime_error("prestressedModes: a start field needs one entry per DoF");
            for (size_t i = 0; i < nDoF; ++i)
                for (size_t a = 0; a < N; ++a) x0[(m * nDoF + i) * N + a] = start[m][i][a];
        }
    }
    check(c, mfh_modes_prestressed(c, nev, density, loadFactor, 0, opt.rtol, opt.maxit, x0.empty() ? nullptr : x0.data(), lambda.data(), flat.data(), nullptr, info));
    std::vector<typename Sim::VField> modes(k, typename Sim::VField(nDoF));
    for (size_t m = 0; m < k; ++m)
        for (size_t i = 0; i < nDoF; ++i)
            for (size_t a = 0; a < N; ++a) modes[m][i][a] = flat[(m * nDoF + i) * N + a];
    return {lambda, modes};
}

} // namespace MeshFEMHip
