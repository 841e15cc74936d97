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

} // namespace MeshFEMHip
