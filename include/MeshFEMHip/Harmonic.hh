// Frequency response on the MI355X path: damped harmonic sweeps over the C ABI (include/meshfem_hip.h, "frequency response"). The reference has no
// harmonic solver, so there is no counterpart to cite; the layout follows Dynamics.hh.
//   frequencyResponse(sim, omegas, opt)   (K + i w C - w^2 M) u^(w) = f^ for every w of omegas (rad per unit time), solved in that order: K = the
//                                         Simulator's stiffness matrix, M = opt.density x the consistent vector-valued mass matrix, C =
//                                         opt.rayleighMass M + opt.rayleighStiff K plus the structural term i opt.lossFactor K, f^ = the Simulator's
//                                         neumannLoad() or opt.load + i opt.loadImag. The Dirichlet variables of the boundary conditions applied to
//                                         the Simulator are the clamp, held at zero.
// Returns one complex field per frequency, the probe values, the COCG iterations and the true residuals ||f^ - Z u^|| / ||f^|| per frequency. COCG on
// the device with the Simulator's preconditioner (mfh_set_preconditioner) on both planes; throws std::runtime_error where the C call fails, a frequency
// that does not reach opt.rtol within opt.maxit iterations included.
#pragma once

#include <algorithm>
#include <complex>
#include <utility>

#include "LinearElasticity.hh"

namespace MeshFEMHip {

template <class VField>
struct HarmonicOptions {
    Real density = 1.0, rayleighMass = 0.0, rayleighStiff = 0.0, lossFactor = 0.0;
    std::vector<Real> elementDensity;                     // one value per element: becomes the context's density field (mfh_set_density; density multiplies it); empty: the field in force
    Real rtol = 1e-8;       // ||r||_2 <= rtol ||f^||_2 at every frequency
    int maxit = 10000;
    VField load, loadImag;                                // f^, one N-vector per DoF; load empty: neumannLoad(); loadImag empty: a real load
    std::vector<std::pair<size_t, int>> probes;           // (DoF, component) pairs recorded at every frequency
    bool fields = true;                                   // false: probes only
    bool warmStart = true;                                // every frequency starts from the previous solution
};

template <size_t N>
struct HarmonicResult {
    using CField = std::vector<std::array<std::complex<Real>, N>>;
    std::vector<CField> u;                                // [nFreq][nDoF]
    std::vector<std::vector<std::complex<Real>>> probes;  // [nFreq][number of probes]
    std::vector<int32_t> iterations;                      // [nFreq]
    std::vector<Real> trueResiduals;                      // [nFreq]
    mfh_harmonic_info info{};
};

template <class Sim>
HarmonicResult<std::tuple_size<typename Sim::VField::value_type>::value>
frequencyResponse(const Sim &sim, const std::vector<Real> &omegas, const HarmonicOptions<typename Sim::VField> &opt = HarmonicOptions<typename Sim::VField>()) {
    using VField = typename Sim::VField;
    constexpr size_t N = std::tuple_size<typename VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    check(c, mfh_clear_fixed(c));
    int64_t nv = 0;
    check(c, mfh_bc_dirichlet_vars(c, nullptr, nullptr, &nv));
    if (nv > 0) {
        std::vector<int64_t> vars((size_t)nv);
        std::vector<Real> vals((size_t)nv);
        check(c, mfh_bc_dirichlet_vars(c, vars.data(), vals.data(), &nv));
        check(c, mfh_fix_variables(c, nv, vars.data(), nullptr));
    }
    if (!opt.elementDensity.empty()) check(c, mfh_set_density(c, opt.elementDensity.data(), (int64_t)opt.elementDensity.size(), 0));
    const size_t nDoF = sim.numDoFs(), n = nDoF * N, nFreq = omegas.size();
    if (!opt.load.empty() && opt.load.size() != nDoF) throw std::runtime_error("frequencyResponse: load needs one entry per DoF");
    if (!opt.loadImag.empty() && opt.loadImag.size() != nDoF) throw std::runtime_error("frequencyResponse: loadImag needs one entry per DoF");
    const VField f = opt.load.empty() ? sim.neumannLoad() : opt.load;
    std::vector<int64_t> probeVars;
    for (const auto &p : opt.probes) probeVars.push_back((int64_t)(p.first * N) + p.second);
    const size_t nProbe = probeVars.size();
    std::vector<Real> probeOut(nFreq * nProbe * 2), fld(opt.fields ? nFreq * 2 * n : 0);
    HarmonicResult<N> r;
    r.iterations.assign(nFreq, 0);
    r.trueResiduals.assign(nFreq, 0.0);
    mfh_harmonic_params prm{};
    prm.density = opt.density; prm.rayleighMass = opt.rayleighMass; prm.rayleighStiff = opt.rayleighStiff; prm.lossFactor = opt.lossFactor;
    prm.rtol = opt.rtol; prm.nFreq = (int32_t)nFreq; prm.maxit = opt.maxit; prm.flags = opt.warmStart ? MFH_HARM_WARM_START : 0;
    check(c, mfh_harmonic(c, &prm, omegas.data(), &f[0][0], opt.loadImag.empty() ? nullptr : &opt.loadImag[0][0], nProbe ? probeVars.data() : nullptr,
                          (int32_t)nProbe, nProbe ? probeOut.data() : nullptr, opt.fields ? fld.data() : nullptr, r.iterations.data(),
                          r.trueResiduals.data(), &r.info));
    r.probes.assign(nFreq, std::vector<std::complex<Real>>(nProbe));
    for (size_t k = 0; k < nFreq; ++k)
        for (size_t j = 0; j < nProbe; ++j) r.probes[k][j] = {probeOut[(k * nProbe + j) * 2], probeOut[(k * nProbe + j) * 2 + 1]};
    if (opt.fields) {
        r.u.assign(nFreq, typename HarmonicResult<N>::CField(nDoF));
        for (size_t k = 0; k < nFreq; ++k)
            for (size_t i = 0; i < nDoF; ++i)
                for (size_t a = 0; a < N; ++a) r.u[k][i][a] = {fld[(2 * k) * n + i * N + a], fld[(2 * k + 1) * n + i * N + a]};
    }
    return r;
}

// ---- the same response by superposition of the lowest modes (include/meshfem_hip.h, "modal superposition"; docs/design/04_21_modal_superposition.md)
//   modalFrequencyResponse(sim, omegas, opt)   u^(w) = sum_j phi_j q_j(w) + r_s / zK(w) on opt.nModes modes computed here (mfh_modes_many) and kept
//                                              on the device (mfh_modal_set_basis), or on the eigenpairs the caller hands in (opt.lambda, opt.modes);
//                                              system, load, clamp, damping and probes as in frequencyResponse. opt.staticCorrection: one static solve
//                                              per load plane at opt.rtol / opt.maxit stands in for the truncated modes (clamped bodies only).
template <class VField>
struct ModalHarmonicOptions {
    Real density = 1.0, rayleighMass = 0.0, rayleighStiff = 0.0, lossFactor = 0.0;
    int nModes = 16;                                      // modes computed here when lambda is empty (1 .. 256)
    int batch = 0;                                        // ... in batches of this many (0: the library's 16)
    Real modesRtol = 1e-6;
    std::vector<Real> lambda;                             // eigenpairs of (K, density M) the caller has: M-orthonormal per-DoF rows, modes[j] = one N-vector per DoF
    std::vector<VField> modes;
    std::vector<Real> modalDamping;                       // damping ratios per mode; empty: none
    bool staticCorrection = true;
    int residualStride = -1;                              // < 0: no true residuals; k >= 0: at every k-th frequency (0: every one)
    Real rtol = 1e-8;                                     // of the static solves
    int maxit = 10000;
    VField load, loadImag;
    std::vector<std::pair<size_t, int>> probes;
    bool fields = true;
};

template <size_t N>
struct ModalHarmonicResult {
    using CField = std::vector<std::array<std::complex<Real>, N>>;
    std::vector<CField> u;                                    // [nFreq][nDoF]
    std::vector<std::vector<std::complex<Real>>> probes;      // [nFreq][number of probes]
    std::vector<std::vector<std::complex<Real>>> modalCoords; // [nFreq][nModes]
    std::vector<Real> trueResiduals;                          // [nFreq], -1 where none was computed
    std::vector<Real> lambda;                                 // the basis's eigenvalues
    mfh_modal_basis_info basisInfo{};
    mfh_modal_harmonic_info info{};
};

template <class Sim>
ModalHarmonicResult<std::tuple_size<typename Sim::VField::value_type>::value>
modalFrequencyResponse(const Sim &sim, const std::vector<Real> &omegas,
                       const ModalHarmonicOptions<typename Sim::VField> &opt = ModalHarmonicOptions<typename Sim::VField>()) {
    using VField = typename Sim::VField;
    constexpr size_t N = std::tuple_size<typename VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    check(c, mfh_clear_fixed(c));
    int64_t nv = 0;
    check(c, mfh_bc_dirichlet_vars(c, nullptr, nullptr, &nv));
    if (nv > 0) {
        std::vector<int64_t> vars((size_t)nv);
        std::vector<Real> vals((size_t)nv);
        check(c, mfh_bc_dirichlet_vars(c, vars.data(), vals.data(), &nv));
        check(c, mfh_fix_variables(c, nv, vars.data(), nullptr));
    }
    const size_t nDoF = sim.numDoFs(), n = nDoF * N, nFreq = omegas.size();
    if (!opt.load.empty() && opt.load.size() != nDoF) throw std::runtime_error("modalFrequencyResponse: load needs one entry per DoF");
    if (!opt.loadImag.empty() && opt.loadImag.size() != nDoF) throw std::runtime_error("modalFrequencyResponse: loadImag needs one entry per DoF");
    ModalHarmonicResult<N> r;
    std::vector<Real> X;
    if (opt.lambda.empty()) {
        mfh_modes_many_params mp{};
        mp.nev = opt.nModes; mp.batch = opt.batch; mp.flags = nv > 0 ? 0 : MFH_MODES_FREE; mp.maxit = 3000;
        mp.density = opt.density; mp.rtol = opt.modesRtol;
        r.lambda.assign((size_t)std::max(opt.nModes, 0), 0.0);
        X.assign(r.lambda.size() * n, 0.0);
        mfh_modes_many_info mi{};
        check(c, mfh_modes_many(c, &mp, nullptr, r.lambda.data(), X.data(), nullptr, &mi));
    } else {
        if (opt.modes.size() != opt.lambda.size()) throw std::runtime_error("modalFrequencyResponse: one mode per eigenvalue");
        r.lambda = opt.lambda;
        X.resize(r.lambda.size() * n);
        for (size_t j = 0; j < opt.modes.size(); ++j) {
            if (opt.modes[j].size() != nDoF) throw std::runtime_error("modalFrequencyResponse: a mode needs one entry per DoF");
            std::copy(&opt.modes[j][0][0], &opt.modes[j][0][0] + n, X.begin() + (std::ptrdiff_t)(j * n));
        }
    }
    const size_t m = r.lambda.size();
    if (!opt.modalDamping.empty() && opt.modalDamping.size() != m) throw std::runtime_error("modalFrequencyResponse: one damping ratio per mode");
    check(c, mfh_modal_set_basis(c, (int32_t)m, r.lambda.data(), X.data(), opt.density, &r.basisInfo));
    const VField f = opt.load.empty() ? sim.neumannLoad() : opt.load;
    std::vector<int64_t> probeVars;
    for (const auto &p : opt.probes) probeVars.push_back((int64_t)(p.first * N) + p.second);
    const size_t nProbe = probeVars.size();
    std::vector<Real> probeOut(nFreq * nProbe * 2), fld(opt.fields ? nFreq * 2 * n : 0), mc(nFreq * m * 2);
    r.trueResiduals.assign(nFreq, -1.0);
    mfh_modal_harmonic_params prm{};
    prm.rayleighMass = opt.rayleighMass; prm.rayleighStiff = opt.rayleighStiff; prm.lossFactor = opt.lossFactor;
    prm.rtol = opt.rtol; prm.maxit = opt.maxit; prm.nFreq = (int32_t)nFreq;
    prm.residualStride = std::max(opt.residualStride, 0);
    prm.flags = (opt.staticCorrection ? MFH_MODAL_STATIC_CORRECTION : 0) | (opt.residualStride >= 0 ? MFH_MODAL_RESIDUALS : 0);
    check(c, mfh_modal_harmonic(c, &prm, omegas.data(), opt.modalDamping.empty() ? nullptr : opt.modalDamping.data(), &f[0][0],
                                opt.loadImag.empty() ? nullptr : &opt.loadImag[0][0], nProbe ? probeVars.data() : nullptr, (int32_t)nProbe,
                                nProbe ? probeOut.data() : nullptr, opt.fields ? fld.data() : nullptr, mc.empty() ? nullptr : mc.data(),
                                r.trueResiduals.data(), &r.info));
    r.probes.assign(nFreq, std::vector<std::complex<Real>>(nProbe));
    r.modalCoords.assign(nFreq, std::vector<std::complex<Real>>(m));
    for (size_t k = 0; k < nFreq; ++k) {
        for (size_t j = 0; j < nProbe; ++j) r.probes[k][j] = {probeOut[(k * nProbe + j) * 2], probeOut[(k * nProbe + j) * 2 + 1]};
        for (size_t j = 0; j < m; ++j) r.modalCoords[k][j] = {mc[(k * m + j) * 2], mc[(k * m + j) * 2 + 1]};
    }
    if (opt.fields) {
        r.u.assign(nFreq, typename ModalHarmonicResult<N>::CField(nDoF));
        for (size_t k = 0; k < nFreq; ++k)
            for (size_t i = 0; i < nDoF; ++i)
                for (size_t a = 0; a < N; ++a) r.u[k][i][a] = {fld[(2 * k) * n + i * N + a], fld[(2 * k + 1) * n + i * N + a]};
    }
    return r;
}

} // namespace MeshFEMHip
