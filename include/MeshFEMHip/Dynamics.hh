// Transient dynamics on the MI355X path: implicit Newmark time stepping over the C ABI (include/meshfem_hip.h, "transient dynamics"). The reference has
// no time integrator, so there is no counterpart to cite; the layout follows Eigensolver.hh.
//   transient(sim, dt, nSteps, opt)   M u'' + C u' + K u = g(t) f with K = the Simulator's stiffness matrix, M = opt.density x the consistent vector-valued
//                                     mass matrix, C = opt.rayleighMass M + opt.rayleighStiff K, f = the Simulator's neumannLoad() or opt.load, g = opt.amplitude (steps
//                                     0 .. nSteps; empty: 1). The Dirichlet variables of the boundary conditions applied to the Simulator are the clamp,
//                                     held at zero. opt.u0 / v0 / a0: the state at step 0, one N-vector per DoF (empty: rest; a0 empty: from the equation
//                                     of motion at step 0 -- pass the a of an earlier result to continue that run).
// Returns the state after the last step, the probe histories, the snapshots (one field per snapshot step) and, if asked for, the energies
// {kinetic, strain, g f.u} per step. PCG on the device with the Simulator's preconditioner (mfh_set_preconditioner); throws std::runtime_error where the C
// call fails, a step whose PCG does not reach opt.rtol within opt.maxit iterations included.
#pragma once

#include <utility>

#include "LinearElasticity.hh"

namespace MeshFEMHip {

namespace detail {
// the Dirichlet variables of the boundary conditions applied to the Simulator become the clamp (transient and explicitTransient)
inline void clampDirichlet(mfh_ctx *c) {
    check(c, mfh_clear_fixed(c));
    int64_t nv = 0;
    check(c, mfh_bc_dirichlet_vars(c, nullptr, nullptr, &nv));
    if (nv > 0) {
        std::vector<int64_t> vars((size_t)nv);
        std::vector<Real> vals((size_t)nv);
        check(c, mfh_bc_dirichlet_vars(c, vars.data(), vals.data(), &nv));
        check(c, mfh_fix_variables(c, nv, vars.data(), nullptr));
    }
}
} // namespace detail

template <class VField>
struct TransientOptions {
    Real density = 1.0, rayleighMass = 0.0, rayleighStiff = 0.0;
    std::vector<Real> elementDensity;                     // one value per element: becomes the context's density field (mfh_set_density; density multiplies it); empty: the field in force
    Real beta = 0.25, gamma = 0.5;
    Real rtol = 1e-8;       // ||r||_2 <= rtol ||b||_2 in every step's solve
    int maxit = 10000;
    std::vector<Real> amplitude;                          // nSteps + 1 values, or empty (= 1)
    VField u0, v0, a0;                                    // one N-vector per DoF, or empty
    VField load;                                          // f, one N-vector per DoF (a volume load of VolumeLoads.hh, a sum of loads); empty: neumannLoad()
    std::vector<std::pair<size_t, int>> probes;           // (DoF, component) pairs recorded at every step
    int snapshotStride = 0;                               // > 0: the displacement at the steps 0, stride, 2 stride, ...
    bool energies = false;
};

template <class VField>
struct TransientResult {
    VField u, v, a;                                       // the state after the last step
    std::vector<std::vector<Real>> probes;                // [nSteps + 1][number of probes]
    std::vector<VField> snapshots;
    std::vector<std::array<Real, 3>> energies;            // [nSteps + 1]: kinetic, strain, g f.u
    mfh_newmark_info info{};
};

template <class Sim>
TransientResult<typename Sim::VField> transient(const Sim &sim, Real dt, int nSteps,
                                                const TransientOptions<typename Sim::VField> &opt = TransientOptions<typename Sim::VField>()) {
    using VField = typename Sim::VField;
    constexpr size_t N = std::tuple_size<typename VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    detail::clampDirichlet(c);
    if (!opt.elementDensity.empty()) check(c, mfh_set_density(c, opt.elementDensity.data(), (int64_t)opt.elementDensity.size(), 0));
    const size_t nDoF = sim.numDoFs(), n = nDoF * N, rows = (size_t)(nSteps > 0 ? nSteps : 0) + 1;
    auto state = [&](const VField &x, const char *name) {
        VField y(nDoF);
        if (!x.empty()) {
            if (x.size() != nDoF) throw std::runtime_error(std::string("transient: ") + name + " needs one entry per DoF");
            y = x;
        } else
            for (auto &e : y) e.fill(0.0);
        return y;
    };
    TransientResult<VField> r;
    r.u = state(opt.u0, "u0"); r.v = state(opt.v0, "v0"); r.a = state(opt.a0, "a0");
    if (!opt.amplitude.empty() && opt.amplitude.size() != rows) throw std::runtime_error("transient: amplitude needs nSteps + 1 values");
    if (!opt.load.empty() && opt.load.size() != nDoF) throw std::runtime_error("transient: load needs one entry per DoF");
    const VField f = opt.load.empty() ? sim.neumannLoad() : opt.load;
    bool loaded = false;
    for (const auto &e : f)
        for (size_t a = 0; a < N; ++a) loaded = loaded || e[a] != 0.0;
    std::vector<int64_t> probeVars;
    for (const auto &p : opt.probes) probeVars.push_back((int64_t)(p.first * N) + p.second);
    std::vector<Real> probeOut(rows * probeVars.size()), snaps, en;
    const size_t nSnap = opt.snapshotStride > 0 ? (rows - 1) / (size_t)opt.snapshotStride + 1 : 0;
    snaps.resize(nSnap * n);
    if (opt.energies) en.resize(rows * 3);
    mfh_newmark_params prm{};
    prm.dt = dt; prm.beta = opt.beta; prm.gamma = opt.gamma; prm.density = opt.density;
    prm.rayleighMass = opt.rayleighMass; prm.rayleighStiff = opt.rayleighStiff; prm.rtol = opt.rtol;
    prm.nSteps = nSteps; prm.maxit = opt.maxit; prm.snapshotStride = nSnap ? opt.snapshotStride : 0;
    prm.flags = (opt.a0.empty() ? 0 : MFH_DYN_HAVE_ACCEL) | (opt.energies ? MFH_DYN_ENERGIES : 0);
    check(c, mfh_newmark(c, &prm, &r.u[0][0], &r.v[0][0], &r.a[0][0], loaded ? &f[0][0] : nullptr, opt.amplitude.empty() ? nullptr : opt.amplitude.data(),
                         probeVars.empty() ? nullptr : probeVars.data(), (int32_t)probeVars.size(), probeVars.empty() ? nullptr : probeOut.data(),
                         nSnap ? snaps.data() : nullptr, opt.energies ? en.data() : nullptr, &r.info));
    r.probes.assign(rows, std::vector<Real>(probeVars.size()));
    for (size_t k = 0; k < rows; ++k)
        for (size_t j = 0; j < probeVars.size(); ++j) r.probes[k][j] = probeOut[k * probeVars.size() + j];
    r.snapshots.assign(nSnap, VField(nDoF));
    for (size_t k = 0; k < nSnap; ++k) std::copy(snaps.begin() + k * n, snaps.begin() + (k + 1) * n, &r.snapshots[k][0][0]);
    r.energies.resize(opt.energies ? rows : 0);
    for (size_t k = 0; k < r.energies.size(); ++k) r.energies[k] = {en[3 * k], en[3 * k + 1], en[3 * k + 2]};
    return r;
}

// ---- explicit dynamics (include/meshfem_hip.h, "explicit dynamics"): central differences with the HRZ-lumped mass matrix -- one product with K per
// step, no solve; for wave propagation, impact and short pulses.
//   stableTimeStep(sim, density, iters)      the stability limit bracketed: dtSafe (stable for certain) and dtEst (an upper bound of the limit, close to
//                                            it) with lambdaUpper >= lambda_max >= lambdaEst of (K, density M_L) on the free variables
//   explicitTransient(sim, nSteps, dt, opt)  M_L u'' + opt.rayleighMass M_L u' + K u = g(t) f; dt <= 0: opt.safety x dtEst. Clamp, load, amplitude, start
//                                            state, probes and snapshots as for transient; energies {kinetic, strain, g f.u, leapfrog invariant} at
//                                            every opt.energyStride-th step. Throws where the C call fails: a step above the stability estimate (unless
//                                            opt.checkDt is false) and a run that blows up included.
template <class VField>
struct ExplicitOptions {
    Real density = 1.0, rayleighMass = 0.0;
    std::vector<Real> elementDensity;                     // one value per element: becomes the context's density field; empty: the field in force
    Real safety = 0.9;                                    // dt <= 0: the step is safety x dtEst
    bool checkDt = true;                                  // false: MFH_EXP_NO_DT_CHECK
    std::vector<Real> amplitude;                          // nSteps + 1 values, or empty (= 1)
    VField u0, v0, a0;                                    // one N-vector per DoF, or empty
    VField load;                                          // f, one N-vector per DoF; empty: neumannLoad()
    std::vector<std::pair<size_t, int>> probes;           // (DoF, component) pairs recorded at every step
    int snapshotStride = 0;                               // > 0: the displacement at the steps 0, stride, 2 stride, ...
    bool energies = false;
    int energyStride = 1;
};

template <class VField>
struct ExplicitResult {
    VField u, v, a;                                       // the state after the last step
    Real dt = 0.0;                                        // the step taken
    std::vector<std::vector<Real>> probes;                // [nSteps + 1][number of probes]
    std::vector<VField> snapshots;
    std::vector<std::array<Real, 4>> energies;            // [nSteps / energyStride + 1]: kinetic, strain, g f.u, the leapfrog invariant
    mfh_explicit_info info{};
};

template <class Sim>
mfh_explicit_dt_info stableTimeStep(const Sim &sim, Real density = 1.0, int iters = 0) {
    mfh_ctx *c = sim.ctx();
    detail::clampDirichlet(c);
    mfh_explicit_dt_info info{};
    check(c, mfh_explicit_dt(c, density, iters, nullptr, &info));
    return info;
}

template <class Sim>
ExplicitResult<typename Sim::VField> explicitTransient(const Sim &sim, int nSteps, Real dt = 0.0,
                                                       const ExplicitOptions<typename Sim::VField> &opt = ExplicitOptions<typename Sim::VField>()) {
    using VField = typename Sim::VField;
    constexpr size_t N = std::tuple_size<typename VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    detail::clampDirichlet(c);
    if (!opt.elementDensity.empty()) check(c, mfh_set_density(c, opt.elementDensity.data(), (int64_t)opt.elementDensity.size(), 0));
    const size_t nDoF = sim.numDoFs(), n = nDoF * N, rows = (size_t)(nSteps > 0 ? nSteps : 0) + 1;
    auto state = [&](const VField &x, const char *name) {
        VField y(nDoF);
        if (!x.empty()) {
            if (x.size() != nDoF) throw std::runtime_error(std::string("explicitTransient: ") + name + " needs one entry per DoF");
            y = x;
        } else
            for (auto &e : y) e.fill(0.0);
        return y;
    };
    ExplicitResult<VField> r;
    r.u = state(opt.u0, "u0"); r.v = state(opt.v0, "v0"); r.a = state(opt.a0, "a0");
    if (!opt.amplitude.empty() && opt.amplitude.size() != rows) throw std::runtime_error("explicitTransient: amplitude needs nSteps + 1 values");
    if (!opt.load.empty() && opt.load.size() != nDoF) throw std::runtime_error("explicitTransient: load needs one entry per DoF");
    if (dt <= 0.0) {
        mfh_explicit_dt_info di{};
        check(c, mfh_explicit_dt(c, opt.density, 0, nullptr, &di));
        dt = opt.safety * di.dtEst;
    }
    r.dt = dt;
    const VField f = opt.load.empty() ? sim.neumannLoad() : opt.load;
    bool loaded = false;
    for (const auto &e : f)
        for (size_t a = 0; a < N; ++a) loaded = loaded || e[a] != 0.0;
    std::vector<int64_t> probeVars;
    for (const auto &p : opt.probes) probeVars.push_back((int64_t)(p.first * N) + p.second);
    std::vector<Real> probeOut(rows * probeVars.size()), snaps, en;
    const size_t nSnap = opt.snapshotStride > 0 ? (rows - 1) / (size_t)opt.snapshotStride + 1 : 0;
    const size_t eStride = (size_t)(opt.energyStride > 0 ? opt.energyStride : 1), nEn = opt.energies ? (rows - 1) / eStride + 1 : 0;
    snaps.resize(nSnap * n);
    en.resize(nEn * 4);
    mfh_explicit_params prm{};
    prm.dt = dt; prm.density = opt.density; prm.rayleighMass = opt.rayleighMass;
    prm.nSteps = nSteps; prm.snapshotStride = nSnap ? opt.snapshotStride : 0; prm.energyStride = (int32_t)eStride;
    prm.flags = (opt.a0.empty() ? 0 : MFH_EXP_HAVE_ACCEL) | (opt.energies ? MFH_EXP_ENERGIES : 0) | (opt.checkDt ? 0 : MFH_EXP_NO_DT_CHECK);
    check(c, mfh_explicit(c, &prm, &r.u[0][0], &r.v[0][0], &r.a[0][0], loaded ? &f[0][0] : nullptr, opt.amplitude.empty() ? nullptr : opt.amplitude.data(),
                          probeVars.empty() ? nullptr : probeVars.data(), (int32_t)probeVars.size(), probeVars.empty() ? nullptr : probeOut.data(),
                          nSnap ? snaps.data() : nullptr, opt.energies ? en.data() : nullptr, &r.info));
    r.probes.assign(rows, std::vector<Real>(probeVars.size()));
    for (size_t k = 0; k < rows; ++k)
        for (size_t j = 0; j < probeVars.size(); ++j) r.probes[k][j] = probeOut[k * probeVars.size() + j];
    r.snapshots.assign(nSnap, VField(nDoF));
    for (size_t k = 0; k < nSnap; ++k) std::copy(snaps.begin() + k * n, snaps.begin() + (k + 1) * n, &r.snapshots[k][0][0]);
    r.energies.resize(nEn);
    for (size_t k = 0; k < nEn; ++k) r.energies[k] = {en[4 * k], en[4 * k + 1], en[4 * k + 2], en[4 * k + 3]};
    return r;
}

// ---- modal transient response (include/meshfem_hip.h, "modal superposition"; docs/design/04_22_modal_transient.md): the load history taken as piecewise
// linear between the steps and every mode of a basis that stays on the device stepped exactly -- no stability limit, no period error.
//   modalTransient(sim, dt, nSteps, opt)   clamp, load, amplitude, probes and snapshots as for transient. The basis: opt.nModes modes computed here
//                                          (mfh_modes_many), or the eigenpairs the caller hands in (opt.lambda, opt.modes), or -- opt.keepBasis -- the one
//                                          an earlier call left on the device. Start: opt.u0 / v0 (projected with mfh_modal_coordinates) or the modal
//                                          state opt.q0 / qdot0 of an earlier result, not both; neither: rest. opt.staticCorrection: one static solve at
//                                          opt.rtol / opt.maxit stands in for the truncated modes (clamped bodies only).
template <class VField>
struct ModalTransientOptions {
    Real density = 1.0, rayleighMass = 0.0, rayleighStiff = 0.0;
    int nModes = 16;                                      // modes computed here when lambda is empty (1 .. 256)
    int batch = 0;
    Real modesRtol = 1e-6;
    bool keepBasis = false;                               // use the basis in place (of an earlier modalTransient / modalFrequencyResponse)
    std::vector<Real> lambda;                             // eigenpairs of (K, density M) the caller has: M-orthonormal per-DoF rows
    std::vector<VField> modes;
    std::vector<Real> modalDamping;                       // damping ratios per mode; empty: none
    bool staticCorrection = true;
    Real rtol = 1e-8;                                     // of the static solve
    int maxit = 10000;
    std::vector<Real> amplitude;                          // nSteps + 1 values, or empty (= 1)
    VField u0, v0;                                        // one N-vector per DoF, or empty
    std::vector<Real> q0, qdot0;                          // the modal state of an earlier result, or empty
    VField load;                                          // f; empty: neumannLoad()
    std::vector<std::pair<size_t, int>> probes;
    int snapshotStride = 0;
    bool modalCoords = false, energies = false;
    int chunkSteps = 0;                                   // steps per launch on the device (0: the default; a multiple of 32); changes no result
};

template <class VField>
struct ModalTransientResult {
    std::vector<Real> q, qdot;                            // the modal state after the last step
    std::vector<std::vector<Real>> probes;                // [nSteps + 1][number of probes]
    std::vector<VField> snapshots;
    std::vector<std::vector<Real>> modalCoords;           // [nSteps + 1][nModes]
    std::vector<std::array<Real, 3>> energies;            // [nSteps + 1]: 1/2 sum qdot^2, 1/2 sum lambda q^2, a sum g q
    mfh_modal_transient_info info{};
};

template <class Sim>
ModalTransientResult<typename Sim::VField> modalTransient(const Sim &sim, Real dt, int nSteps,
                                                          const ModalTransientOptions<typename Sim::VField> &opt = ModalTransientOptions<typename Sim::VField>()) {
    using VField = typename Sim::VField;
    constexpr size_t N = std::tuple_size<typename VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    const size_t nDoF = sim.numDoFs(), n = nDoF * N, rows = (size_t)(nSteps > 0 ? nSteps : 0) + 1;
    if (!opt.keepBasis) {
        detail::clampDirichlet(c);
        int64_t nv = 0;
        check(c, mfh_bc_dirichlet_vars(c, nullptr, nullptr, &nv));
        std::vector<Real> lambda, X;
        if (opt.lambda.empty()) {
            mfh_modes_many_params mp{};
            mp.nev = opt.nModes; mp.batch = opt.batch; mp.flags = nv > 0 ? 0 : MFH_MODES_FREE; mp.maxit = 3000;
            mp.density = opt.density; mp.rtol = opt.modesRtol;
            lambda.assign((size_t)std::max(opt.nModes, 0), 0.0);
            X.assign(lambda.size() * n, 0.0);
            mfh_modes_many_info mi{};
            check(c, mfh_modes_many(c, &mp, nullptr, lambda.data(), X.data(), nullptr, &mi));
        } else {
            if (opt.modes.size() != opt.lambda.size()) throw std::runtime_error("modalTransient: one mode per eigenvalue");
            lambda = opt.lambda;
            X.resize(lambda.size() * n);
            for (size_t j = 0; j < opt.modes.size(); ++j) {
                if (opt.modes[j].size() != nDoF) throw std::runtime_error("modalTransient: a mode needs one entry per DoF");
                std::copy(&opt.modes[j][0][0], &opt.modes[j][0][0] + n, X.begin() + (std::ptrdiff_t)(j * n));
            }
        }
        mfh_modal_basis_info bi{};
        check(c, mfh_modal_set_basis(c, (int32_t)lambda.size(), lambda.data(), X.data(), opt.density, &bi));
    }
    int32_t mm = 0, valid = 0;
    check(c, mfh_modal_basis_state(c, &mm, &valid));
    const size_t m = (size_t)mm;
    if (!opt.modalDamping.empty() && opt.modalDamping.size() != m) throw std::runtime_error("modalTransient: one damping ratio per mode");
    if ((!opt.q0.empty() || !opt.qdot0.empty()) && (!opt.u0.empty() || !opt.v0.empty())) throw std::runtime_error("modalTransient: the start is q0 / qdot0 or u0 / v0, not both");
    if (!opt.amplitude.empty() && opt.amplitude.size() != rows) throw std::runtime_error("modalTransient: amplitude needs nSteps + 1 values");
    if (!opt.load.empty() && opt.load.size() != nDoF) throw std::runtime_error("modalTransient: load needs one entry per DoF");
    ModalTransientResult<VField> r;
    r.q.assign(m, 0.0); r.qdot.assign(m, 0.0);
    auto modal = [&](const std::vector<Real> &x, std::vector<Real> &y, const char *name) {
        if (x.empty()) return;
        if (x.size() != m) throw std::runtime_error(std::string("modalTransient: ") + name + " needs one entry per mode");
        y = x;
    };
    modal(opt.q0, r.q, "q0"); modal(opt.qdot0, r.qdot, "qdot0");
    auto project = [&](const VField &x, std::vector<Real> &y, const char *name) {
        if (x.empty()) return;
        if (x.size() != nDoF) throw std::runtime_error(std::string("modalTransient: ") + name + " needs one entry per DoF");
        check(c, mfh_modal_coordinates(c, &x[0][0], 1, y.data()));
    };
    project(opt.u0, r.q, "u0"); project(opt.v0, r.qdot, "v0");
    const VField f = opt.load.empty() ? sim.neumannLoad() : opt.load;
    std::vector<int64_t> probeVars;
    for (const auto &p : opt.probes) probeVars.push_back((int64_t)(p.first * N) + p.second);
    const size_t nProbe = probeVars.size(), nSnap = opt.snapshotStride > 0 ? (rows - 1) / (size_t)opt.snapshotStride + 1 : 0;
    std::vector<Real> probeOut(rows * nProbe), snaps(nSnap * n), mc(opt.modalCoords ? rows * m : 0), en(opt.energies ? rows * 3 : 0);
    mfh_modal_transient_params prm{};
    prm.dt = dt; prm.rayleighMass = opt.rayleighMass; prm.rayleighStiff = opt.rayleighStiff; prm.rtol = opt.rtol;
    prm.nSteps = nSteps; prm.maxit = opt.maxit; prm.snapshotStride = nSnap ? opt.snapshotStride : 0; prm.chunkSteps = opt.chunkSteps;
    prm.flags = (opt.staticCorrection ? MFH_MODAL_TR_STATIC_CORRECTION : 0) | (opt.energies ? MFH_MODAL_TR_ENERGIES : 0);
    check(c, mfh_modal_transient(c, &prm, opt.modalDamping.empty() ? nullptr : opt.modalDamping.data(), m ? r.q.data() : nullptr, m ? r.qdot.data() : nullptr,
                                 &f[0][0], opt.amplitude.empty() ? nullptr : opt.amplitude.data(), nProbe ? probeVars.data() : nullptr, (int32_t)nProbe,
                                 nProbe ? probeOut.data() : nullptr, nSnap ? snaps.data() : nullptr, mc.empty() ? nullptr : mc.data(),
                                 opt.energies ? en.data() : nullptr, &r.info));
    r.probes.assign(rows, std::vector<Real>(nProbe));
    for (size_t k = 0; k < rows; ++k)
        for (size_t j = 0; j < nProbe; ++j) r.probes[k][j] = probeOut[k * nProbe + j];
    r.snapshots.assign(nSnap, VField(nDoF));
    for (size_t k = 0; k < nSnap; ++k) std::copy(snaps.begin() + k * n, snaps.begin() + (k + 1) * n, &r.snapshots[k][0][0]);
    if (opt.modalCoords) {
        r.modalCoords.assign(rows, std::vector<Real>(m));
        for (size_t k = 0; k < rows; ++k) std::copy(mc.begin() + k * m, mc.begin() + (k + 1) * m, r.modalCoords[k].begin());
    }
    r.energies.resize(opt.energies ? rows : 0);
    for (size_t k = 0; k < r.energies.size(); ++k) r.energies[k] = {en[3 * k], en[3 * k + 1], en[3 * k + 2]};
    return r;
}

} // namespace MeshFEMHip
