// Vibrational modes on the MI355X path: the facade of the reference's Eigensolver.hh over the C ABI (include/meshfem_hip.h, "vibrational modes").
//   reference                                                       here
//   smallestNonzeroGenEigenpairsPSDKnownKernel(K, M, Z, k)           vibrationalModes(sim, nev, density, free = true): K = the Simulator's stiffness
//     (shift-invert Lanczos over CHOLMOD in the M-orthogonal           matrix, M = density x the consistent vector-valued mass matrix, Z = the rigid-body
//      complement of the known kernel Z)                               modes of the mesh, built by the library from the node positions
//   the same pencil with Dirichlet variables removed                 vibrationalModes(sim, nev, density, free = false): the Dirichlet variables of the
//                                                                      boundary conditions applied to the Simulator are the clamp
//   largest eigenvalues, negativeCurvatureDirection                  not offered
//   (no counterpart: the reference's M is at unit density)           vibrationalModes(sim, nev, elementDensity, free): one density per element
//   (no counterpart: more modes than one block of the loop holds)    vibrationalModes(sim, nev, density, free, ManyModesOptions, locked): up to 256 modes
//                                                                      in batches locked on the device (mfh_modes_many), optionally all below
//                                                                      lambdaMax, in the M-orthogonal complement of `locked` (e.g. an earlier call's modes)
// Returns {lambda (ascending, nev), modes (nev fields of one N-vector per DoF, M-orthonormal, largest entry positive)}; the natural frequencies are
// sqrt(lambda) / 2 pi. LOBPCG on the device with the Simulator's preconditioner (mfh_set_preconditioner); throws std::runtime_error where the C
// call fails, a tolerance that maxit iterations do not reach included.
#pragma once

#include <utility>

#include "LinearElasticity.hh"

namespace MeshFEMHip {

struct ModesOptions {
    Real rtol = 1e-6;       // ||K x - lambda M x|| / (lambda ||M x||) per mode
    int maxit = 500;
};

template <class Sim>
std::pair<std::vector<Real>, std::vector<typename Sim::VField>> vibrationalModes(const Sim &sim, int nev, Real density = 1.0, bool free = false,
                                                                                 const ModesOptions &opt = ModesOptions(), mfh_modes_info *info = nullptr) {
    constexpr size_t N = std::tuple_size<typename Sim::VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    check(c, mfh_clear_fixed(c));
    if (!free) {
        int64_t nv = 0;
        check(c, mfh_bc_dirichlet_vars(c, nullptr, nullptr, &nv));
        std::vector<int64_t> vars((size_t)nv);
        std::vector<Real> vals((size_t)nv);
        if (nv > 0) {
            check(c, mfh_bc_dirichlet_vars(c, vars.data(), vals.data(), &nv));
            check(c, mfh_fix_variables(c, nv, vars.data(), nullptr));
        }
    }
    const size_t nDoF = sim.numDoFs(), k = nev > 0 ? (size_t)nev : 0;
    std::vector<Real> lambda(k), flat(k * nDoF * N);
    check(c, mfh_modes(c, nev, density, free ? MFH_MODES_FREE : 0, opt.rtol, opt.maxit, lambda.data(), flat.data(), nullptr, info));
    std::vector<typename Sim::VField> modes(k, typename Sim::VField(nDoF));
    for (size_t m = 0; m < k; ++m)
        for (size_t i = 0; i < nDoF; ++i)
            for (size_t a = 0; a < N; ++a) modes[m][i][a] = flat[(m * nDoF + i) * N + a];
    return {lambda, modes};
}

// the same with one density per element: the field becomes the context's (mfh_set_density, MassProperties.hh) and stays in force after the call
template <class Sim>
std::pair<std::vector<Real>, std::vector<typename Sim::VField>> vibrationalModes(const Sim &sim, int nev, const std::vector<Real> &elementDensity,
                                                                                 bool free = false, const ModesOptions &opt = ModesOptions(),
                                                                                 mfh_modes_info *info = nullptr) {
    mfh_ctx *c = sim.ctx();
    check(c, mfh_set_density(c, elementDensity.data(), (int64_t)elementDensity.size(), 0));
    return vibrationalModes(sim, nev, Real(1.0), free, opt, info);
}

// More modes than one block holds (mfh_modes_many; docs/design/04_19_many_modes.md): batch by batch, every finished batch locked on the device.
struct ManyModesOptions {
    Real rtol = 1e-6;
    int maxit = 500;        // per batch
    int batch = 0;          // modes per batch, 1 .. 20; 0: 16
    Real lockFactor = 0.1;  // batches that get locked run to rtol * lockFactor
    Real lambdaMax = 0;     // > 0: stop once the band [0, lambdaMax] is exhausted and return the modes inside it
};

// {lambda, modes} with info->nFound entries each (nev unless lambdaMax cut the list short); locked: fields the modes stay M-orthogonal to
template <class Sim>
std::pair<std::vector<Real>, std::vector<typename Sim::VField>> vibrationalModes(const Sim &sim, int nev, Real density, bool free, const ManyModesOptions &opt,
                                                                                 const std::vector<typename Sim::VField> &locked = {},
                                                                                 mfh_modes_many_info *info = nullptr) {
    constexpr size_t N = std::tuple_size<typename Sim::VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    check(c, mfh_clear_fixed(c));
    if (!free) {
        int64_t nv = 0;
        check(c, mfh_bc_dirichlet_vars(c, nullptr, nullptr, &nv));
        std::vector<int64_t> vars((size_t)nv);
        std::vector<Real> vals((size_t)nv);
        if (nv > 0) {
            check(c, mfh_bc_dirichlet_vars(c, vars.data(), vals.data(), &nv));
            check(c, mfh_fix_variables(c, nv, vars.data(), nullptr));
        }
    }
    const size_t nDoF = sim.numDoFs(), k = nev > 0 ? (size_t)nev : 0;
    std::vector<Real> q(locked.size() * nDoF * N);
    for (size_t m = 0; m < locked.size(); ++m) {
        if (locked[m].size() != nDoF) throw std::runtime_error("vibrationalModes: a locked field needs one vector per DoF");
        for (size_t i = 0; i < nDoF; ++i)
            for (size_t a = 0; a < N; ++a) q[(m * nDoF + i) * N + a] = locked[m][i][a];
    }
    mfh_modes_many_params prm{};
    prm.nev = nev; prm.nLocked = (int32_t)locked.size(); prm.batch = opt.batch; prm.flags = free ? MFH_MODES_FREE : 0; prm.maxit = opt.maxit;
    prm.density = density; prm.rtol = opt.rtol; prm.lambdaMax = opt.lambdaMax; prm.lockFactor = opt.lockFactor;
    mfh_modes_many_info mine{};
    std::vector<Real> lambda(k), flat(k * nDoF * N);
    check(c, mfh_modes_many(c, &prm, locked.empty() ? nullptr : q.data(), lambda.data(), flat.data(), nullptr, &mine));
    if (info) *info = mine;
    const size_t found = (size_t)mine.nFound;
    lambda.resize(found);
    std::vector<typename Sim::VField> modes(found, typename Sim::VField(nDoF));
    for (size_t m = 0; m < found; ++m)
        for (size_t i = 0; i < nDoF; ++i)
            for (size_t a = 0; a < N; ++a) modes[m][i][a] = flat[(m * nDoF + i) * N + a];
    return {lambda, modes};
}

} // namespace MeshFEMHip
