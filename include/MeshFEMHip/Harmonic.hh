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

// ---- random vibration and response spectra on the same basis (include/meshfem_hip.h, "Random vibration and response spectra";
// docs/design/04_23_modal_random.md)
//   modalRandomResponse(sim, omegas, S, opt)   the RMS displacement (velocity, acceleration on request) under the loads opt.loads (empty: the Neumann
//                                              load) whose amplitudes have the one-sided cross-spectral density S ([nFreq][nLoad][nLoad], Hermitian) on
//                                              the strictly ascending grid omegas; zero-crossing rates and response spectra at the probes
//   responseSpectrum(sim, direction, Sd, opt)  the peak field sqrt(phi_i^T C phi_i), C_jk = rho_jk a_j a_k, a_j = Gamma_j Sd_j, under a base motion in
//                                              `direction`; rule SRSS (rho = I) or CQC (mfh_cqc_matrix)
// Basis, clamp and probes as in modalFrequencyResponse.
namespace detail {
// the clamp of the Dirichlet conditions and the basis: opt.nModes modes computed here, or the caller's eigenpairs
template <class Sim, class Opt>
void setModalBasis(const Sim &sim, const Opt &opt, const char *who, std::vector<Real> &lambda, mfh_modal_basis_info &basisInfo) {
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
    const size_t nDoF = sim.numDoFs(), n = nDoF * N;
    std::vector<Real> X;
    if (opt.lambda.empty()) {
        mfh_modes_many_params mp{};
        mp.nev = opt.nModes; mp.batch = opt.batch; mp.flags = nv > 0 ? 0 : MFH_MODES_FREE; mp.maxit = 3000;
        mp.density = opt.density; mp.rtol = opt.modesRtol;
        lambda.assign((size_t)std::max(opt.nModes, 0), 0.0);
        X.assign(lambda.size() * n, 0.0);
        mfh_modes_many_info mi{};
        check(c, mfh_modes_many(c, &mp, nullptr, lambda.data(), X.data(), nullptr, &mi));
    } else {
        if (opt.modes.size() != opt.lambda.size()) throw std::runtime_error(std::string(who) + ": one mode per eigenvalue");
        lambda = opt.lambda;
        X.resize(lambda.size() * n);
        for (size_t j = 0; j < opt.modes.size(); ++j) {
            if (opt.modes[j].size() != nDoF) throw std::runtime_error(std::string(who) + ": a mode needs one entry per DoF");
            std::copy(&opt.modes[j][0][0], &opt.modes[j][0][0] + n, X.begin() + (std::ptrdiff_t)(j * n));
        }
    }
    check(c, mfh_modal_set_basis(c, (int32_t)lambda.size(), lambda.data(), X.data(), opt.density, &basisInfo));
}
} // namespace detail

template <class VField>
struct ModalRandomOptions {
    Real density = 1.0, rayleighMass = 0.0, rayleighStiff = 0.0, lossFactor = 0.0;
    int nModes = 16, batch = 0;                           // as in ModalHarmonicOptions
    Real modesRtol = 1e-6;
    std::vector<Real> lambda;
    std::vector<VField> modes;
    std::vector<Real> modalDamping;                       // damping ratios per mode; empty: none
    bool staticCorrection = true;                         // at most two loads with it
    bool velocity = false, acceleration = false;          // sigma_v, sigma_a fields as well
    Real tol = -1.0;                                      // of the factorisation (< 0: nb eps max diag)
    Real rtol = 1e-8;                                     // of the static solves
    int maxit = 10000;
    std::vector<VField> loads;                            // the load shapes; empty: the Neumann load
    std::vector<Real> weights;                            // quadrature weights; empty: the trapezoid rule
    std::vector<std::pair<size_t, int>> probes;
    bool fields = true, probePsd = false;
};

template <size_t N>
struct ModalRandomResult {
    using Field = std::vector<std::array<Real, N>>;
    Field sigmaU, sigmaV, sigmaA;                             // [nDoF]; empty where not asked for
    std::vector<Real> probeSigmaU, probeSigmaV, probeSigmaA, probeNu0;   // [number of probes]
    std::vector<std::vector<Real>> probePsd;                  // [number of probes][nFreq]
    std::array<std::vector<Real>, 3> cov;                     // C^(0), C^(2), C^(4): nb x nb row-major
    std::vector<Real> lambda;
    mfh_modal_basis_info basisInfo{};
    mfh_modal_random_info info{};
};

template <class Sim>
ModalRandomResult<std::tuple_size<typename Sim::VField::value_type>::value>
modalRandomResponse(const Sim &sim, const std::vector<Real> &omegas, const std::vector<std::complex<Real>> &S,
                    const ModalRandomOptions<typename Sim::VField> &opt = ModalRandomOptions<typename Sim::VField>()) {
    using VField = typename Sim::VField;
    constexpr size_t N = std::tuple_size<typename VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    const size_t nDoF = sim.numDoFs(), n = nDoF * N, nFreq = omegas.size(), nLoad = std::max<size_t>(opt.loads.size(), 1);
    if (S.size() != nFreq * nLoad * nLoad) throw std::runtime_error("modalRandomResponse: S needs nFreq x nLoad x nLoad entries");
    if (!opt.weights.empty() && opt.weights.size() != nFreq) throw std::runtime_error("modalRandomResponse: one weight per frequency");
    ModalRandomResult<N> r;
    detail::setModalBasis(sim, opt, "modalRandomResponse", r.lambda, r.basisInfo);
    const size_t m = r.lambda.size();
    if (!opt.modalDamping.empty() && opt.modalDamping.size() != m) throw std::runtime_error("modalRandomResponse: one damping ratio per mode");
    std::vector<Real> f(nLoad * n);
    if (opt.loads.empty()) {
        const VField l = sim.neumannLoad();
        std::copy(&l[0][0], &l[0][0] + n, f.begin());
    } else
        for (size_t a = 0; a < nLoad; ++a) {
            if (opt.loads[a].size() != nDoF) throw std::runtime_error("modalRandomResponse: a load needs one entry per DoF");
            std::copy(&opt.loads[a][0][0], &opt.loads[a][0][0] + n, f.begin() + (std::ptrdiff_t)(a * n));
        }
    std::vector<int64_t> probeVars;
    for (const auto &p : opt.probes) probeVars.push_back((int64_t)(p.first * N) + p.second);
    const size_t nProbe = probeVars.size(), planes = 1 + (opt.velocity ? 1 : 0) + (opt.acceleration ? 1 : 0), nbMax = m + 2;
    std::vector<Real> rms(4 * nProbe), psd(opt.probePsd ? nProbe * nFreq : 0), fld(opt.fields ? planes * n : 0), cov(3 * nbMax * nbMax);
    mfh_modal_random_params prm{};
    prm.rayleighMass = opt.rayleighMass; prm.rayleighStiff = opt.rayleighStiff; prm.lossFactor = opt.lossFactor;
    prm.rtol = opt.rtol; prm.tol = opt.tol; prm.maxit = opt.maxit; prm.nFreq = (int32_t)nFreq; prm.nLoad = (int32_t)nLoad;
    prm.flags = (opt.staticCorrection ? MFH_MODAL_RV_STATIC_CORRECTION : 0) | (opt.velocity ? MFH_MODAL_RV_VELOCITY : 0) |
                (opt.acceleration ? MFH_MODAL_RV_ACCELERATION : 0);
    check(c, mfh_modal_random(c, &prm, omegas.data(), opt.weights.empty() ? nullptr : opt.weights.data(),
                              opt.modalDamping.empty() ? nullptr : opt.modalDamping.data(), f.data(), reinterpret_cast<const Real *>(S.data()),
                              nProbe ? probeVars.data() : nullptr, (int32_t)nProbe, nProbe ? rms.data() : nullptr,
                              (opt.probePsd && nProbe) ? psd.data() : nullptr, opt.fields ? fld.data() : nullptr, cov.data(), &r.info));
    const size_t nb = (size_t)r.info.nb;
    for (size_t q = 0; q < 3; ++q) r.cov[q].assign(cov.begin() + (std::ptrdiff_t)(q * nb * nb), cov.begin() + (std::ptrdiff_t)((q + 1) * nb * nb));
    if (nProbe) {
        r.probeSigmaU.assign(rms.begin(), rms.begin() + (std::ptrdiff_t)nProbe);
        r.probeSigmaV.assign(rms.begin() + (std::ptrdiff_t)nProbe, rms.begin() + (std::ptrdiff_t)(2 * nProbe));
        if (opt.acceleration) r.probeSigmaA.assign(rms.begin() + (std::ptrdiff_t)(2 * nProbe), rms.begin() + (std::ptrdiff_t)(3 * nProbe));
        r.probeNu0.assign(rms.begin() + (std::ptrdiff_t)(3 * nProbe), rms.end());
        if (opt.probePsd)
            for (size_t p = 0; p < nProbe; ++p) r.probePsd.emplace_back(psd.begin() + (std::ptrdiff_t)(p * nFreq), psd.begin() + (std::ptrdiff_t)((p + 1) * nFreq));
    }
    if (opt.fields) {
        typename ModalRandomResult<N>::Field *dst[3] = {&r.sigmaU, opt.velocity ? &r.sigmaV : nullptr, opt.acceleration ? &r.sigmaA : nullptr};
        size_t plane = 0;
        for (auto *d : dst) {
            if (!d) continue;
            d->resize(nDoF);
            std::copy(fld.begin() + (std::ptrdiff_t)(plane * n), fld.begin() + (std::ptrdiff_t)((plane + 1) * n), &(*d)[0][0]);
            ++plane;
        }
    }
    return r;
}

template <class VField>
struct ResponseSpectrumOptions {
    Real density = 1.0;
    int nModes = 16, batch = 0;
    Real modesRtol = 1e-6;
    std::vector<Real> lambda;
    std::vector<VField> modes;
    Real zeta = 0.05;                                     // damping ratio of every mode, or ...
    std::vector<Real> modalDamping;                       // ... one per mode
    bool cqc = true;                                      // false: SRSS
    Real tol = -1.0;
    std::vector<std::pair<size_t, int>> probes;
    bool fields = true;
};

template <size_t N>
struct ResponseSpectrumResult {
    std::vector<std::array<Real, N>> R;                       // [nDoF]; empty without fields
    std::vector<Real> probes, gamma, a, lambda;               // peak values at the probes; participation factors; a_j = gamma_j Sd_j
    Real massFraction = 0.0;                                  // sum_j gamma_j^2 over the moving mass r_f^T (density M) r_f
    mfh_modal_basis_info basisInfo{};
    mfh_modal_quadratic_info info{};
};

// Sd: the spectral displacement as a function of (omega_j, zeta_j)
template <class Sim, class SdFn>
ResponseSpectrumResult<std::tuple_size<typename Sim::VField::value_type>::value>
responseSpectrum(const Sim &sim, int direction, SdFn Sd, const ResponseSpectrumOptions<typename Sim::VField> &opt = ResponseSpectrumOptions<typename Sim::VField>()) {
    using VField = typename Sim::VField;
    constexpr size_t N = std::tuple_size<typename VField::value_type>::value;
    if (direction < 0 || direction >= (int)N) throw std::runtime_error("responseSpectrum: direction out of range");
    mfh_ctx *c = sim.ctx();
    const size_t nDoF = sim.numDoFs(), n = nDoF * N;
    ResponseSpectrumResult<N> r;
    detail::setModalBasis(sim, opt, "responseSpectrum", r.lambda, r.basisInfo);
    const size_t m = r.lambda.size();
    if (!opt.modalDamping.empty() && opt.modalDamping.size() != m) throw std::runtime_error("responseSpectrum: one damping ratio per mode");
    std::vector<Real> zeta = opt.modalDamping.empty() ? std::vector<Real>(m, opt.zeta) : opt.modalDamping;
    std::vector<Real> rd(n, 0.0), Mr(n, 0.0);
    for (size_t i = 0; i < nDoF; ++i) rd[i * N + (size_t)direction] = 1.0;
    r.gamma.assign(m, 0.0);
    check(c, mfh_modal_coordinates(c, rd.data(), 1, r.gamma.data()));
    int64_t nv = 0;
    check(c, mfh_bc_dirichlet_vars(c, nullptr, nullptr, &nv));
    if (nv > 0) {
        std::vector<int64_t> vars((size_t)nv);
        std::vector<Real> vals((size_t)nv);
        check(c, mfh_bc_dirichlet_vars(c, vars.data(), vals.data(), &nv));
        for (int64_t v : vars) rd[(size_t)v] = 0.0;
    }
    check(c, mfh_mass_apply(c, rd.data(), Mr.data(), 0));
    Real moving = 0.0, reached = 0.0;
    for (size_t i = 0; i < n; ++i) moving += rd[i] * Mr[i];
    r.a.assign(m, 0.0);
    for (size_t j = 0; j < m; ++j) { r.a[j] = r.gamma[j] * Sd(std::sqrt(r.lambda[j]), zeta[j]); reached += r.gamma[j] * r.gamma[j]; }
    r.massFraction = moving > 0.0 ? reached / (opt.density * moving) : 0.0;
    std::vector<Real> C(m * m, 0.0);
    if (opt.cqc) check(c, mfh_cqc_matrix((int32_t)m, r.lambda.data(), zeta.data(), C.data()));
    else for (size_t j = 0; j < m; ++j) C[j * m + j] = 1.0;
    for (size_t j = 0; j < m; ++j)
        for (size_t k = 0; k < m; ++k) C[j * m + k] *= r.a[j] * r.a[k];
    std::vector<int64_t> probeVars;
    for (const auto &p : opt.probes) probeVars.push_back((int64_t)(p.first * N) + p.second);
    const size_t nProbe = probeVars.size();
    r.probes.assign(nProbe, 0.0);
    std::vector<Real> fld(opt.fields ? n : 0);
    check(c, mfh_modal_quadratic(c, 1, C.data(), opt.tol, nProbe ? probeVars.data() : nullptr, (int32_t)nProbe, nProbe ? r.probes.data() : nullptr,
                                 opt.fields ? fld.data() : nullptr, &r.info));
    if (opt.fields) {
        r.R.resize(nDoF);
        std::copy(fld.begin(), fld.end(), &r.R[0][0]);
    }
    return r;
}

// ---- RMS stress (mfh_modal_random_stress, mfh_modal_quadratic_stress; docs/design/04_24_modal_stress.md). Per element corner, stressField's layout:
// vonMises [nElem * NQ] = sqrt(E[sigma_vm^2]) (Segalman: the root of the mean square of the von Mises stress, not its mean), components
// [nElem * NQ * flatLen] = sqrt(E[sigma_c^2]); NQ = 1 for degree 1 and N + 1 for degree 2.
struct ModalStressOptions {
    bool vonMises = true, components = false, strain = false;      // strain: strains instead of stresses
    int32_t flags() const {
        return (vonMises ? MFH_MODAL_STRESS_VON_MISES : 0) | (components ? MFH_MODAL_STRESS_COMPONENTS : 0) | (strain ? MFH_MODAL_STRESS_STRAIN : 0);
    }
};

struct ModalStressResult {
    std::vector<Real> vonMises, components;                   // empty where not asked for
    Real peakVonMises = 0.0;
    size_t peakElement = 0, peakCorner = 0;
    std::vector<Real> cov;                                    // modalRandomStress: C^(0), nb x nb row-major
    std::vector<Real> gamma, a;                               // responseSpectrumStress: participation factors, a_j = gamma_j Sd_j
    std::vector<Real> lambda;
    mfh_modal_basis_info basisInfo{};
    mfh_modal_stress_info info{};
};

namespace detail {
template <size_t N, size_t Deg>
constexpr size_t stressNQ(const LinearElasticity::Simulator<N, Deg> &) { return Deg == 1 ? 1 : N + 1; }
template <class Sim>
size_t stressCorners(const Sim &sim) { return sim.numElements() * stressNQ(sim); }
inline void setStressPeak(ModalStressResult &r, size_t nq) {
    r.peakVonMises = r.info.peakVonMises[0];
    r.peakElement = (size_t)r.info.peakCorner[0] / nq;
    r.peakCorner = (size_t)r.info.peakCorner[0] % nq;
}
}   // namespace detail

// the loads, spectrum, basis and damping of modalRandomResponse (its velocity / acceleration / probe options are not used)
template <class Sim>
ModalStressResult modalRandomStress(const Sim &sim, const std::vector<Real> &omegas, const std::vector<std::complex<Real>> &S,
                                    const ModalRandomOptions<typename Sim::VField> &opt = ModalRandomOptions<typename Sim::VField>(),
                                    const ModalStressOptions &sopt = ModalStressOptions()) {
    using VField = typename Sim::VField;
    constexpr size_t N = std::tuple_size<typename VField::value_type>::value, FL = N * (N + 1) / 2;
    mfh_ctx *c = sim.ctx();
    const size_t nDoF = sim.numDoFs(), n = nDoF * N, nFreq = omegas.size(), nLoad = std::max<size_t>(opt.loads.size(), 1);
    if (S.size() != nFreq * nLoad * nLoad) throw std::runtime_error("modalRandomStress: S needs nFreq x nLoad x nLoad entries");
    if (!opt.weights.empty() && opt.weights.size() != nFreq) throw std::runtime_error("modalRandomStress: one weight per frequency");
    ModalStressResult r;
    detail::setModalBasis(sim, opt, "modalRandomStress", r.lambda, r.basisInfo);
    const size_t m = r.lambda.size();
    if (!opt.modalDamping.empty() && opt.modalDamping.size() != m) throw std::runtime_error("modalRandomStress: one damping ratio per mode");
    std::vector<Real> f(nLoad * n);
    if (opt.loads.empty()) {
        const VField l = sim.neumannLoad();
        std::copy(&l[0][0], &l[0][0] + n, f.begin());
    } else
        for (size_t a = 0; a < nLoad; ++a) {
            if (opt.loads[a].size() != nDoF) throw std::runtime_error("modalRandomStress: a load needs one entry per DoF");
            std::copy(&opt.loads[a][0][0], &opt.loads[a][0][0] + n, f.begin() + (std::ptrdiff_t)(a * n));
        }
    const size_t corners = detail::stressCorners(sim), nbMax = m + 2;
    r.vonMises.assign(sopt.vonMises ? corners : 0, 0.0);
    r.components.assign(sopt.components ? corners * FL : 0, 0.0);
    std::vector<Real> cov(nbMax * nbMax);
    mfh_modal_random_params prm{};
    prm.rayleighMass = opt.rayleighMass; prm.rayleighStiff = opt.rayleighStiff; prm.lossFactor = opt.lossFactor;
    prm.rtol = opt.rtol; prm.tol = opt.tol; prm.maxit = opt.maxit; prm.nFreq = (int32_t)nFreq; prm.nLoad = (int32_t)nLoad;
    prm.flags = opt.staticCorrection ? MFH_MODAL_RV_STATIC_CORRECTION : 0;
    check(c, mfh_modal_random_stress(c, &prm, omegas.data(), opt.weights.empty() ? nullptr : opt.weights.data(),
                                     opt.modalDamping.empty() ? nullptr : opt.modalDamping.data(), f.data(), reinterpret_cast<const Real *>(S.data()),
                                     sopt.flags(), sopt.vonMises ? r.vonMises.data() : nullptr, sopt.components ? r.components.data() : nullptr, cov.data(),
                                     &r.info));
    const size_t nb = (size_t)r.info.nb;
    r.cov.assign(cov.begin(), cov.begin() + (std::ptrdiff_t)(nb * nb));
    detail::setStressPeak(r, detail::stressNQ(sim));
    return r;
}

// the base motion, a_j = gamma_j Sd_j and the rules of responseSpectrum (its probe / fields options are not used)
template <class Sim, class SdFn>
ModalStressResult responseSpectrumStress(const Sim &sim, int direction, SdFn Sd,
                                         const ResponseSpectrumOptions<typename Sim::VField> &opt = ResponseSpectrumOptions<typename Sim::VField>(),
                                         const ModalStressOptions &sopt = ModalStressOptions()) {
    using VField = typename Sim::VField;
    constexpr size_t N = std::tuple_size<typename VField::value_type>::value, FL = N * (N + 1) / 2;
    if (direction < 0 || direction >= (int)N) throw std::runtime_error("responseSpectrumStress: direction out of range");
    mfh_ctx *c = sim.ctx();
    const size_t nDoF = sim.numDoFs(), n = nDoF * N;
    ModalStressResult r;
    detail::setModalBasis(sim, opt, "responseSpectrumStress", r.lambda, r.basisInfo);
    const size_t m = r.lambda.size();
    if (!opt.modalDamping.empty() && opt.modalDamping.size() != m) throw std::runtime_error("responseSpectrumStress: one damping ratio per mode");
    std::vector<Real> zeta = opt.modalDamping.empty() ? std::vector<Real>(m, opt.zeta) : opt.modalDamping;
    std::vector<Real> rd(n, 0.0);
    for (size_t i = 0; i < nDoF; ++i) rd[i * N + (size_t)direction] = 1.0;
    r.gamma.assign(m, 0.0);
    check(c, mfh_modal_coordinates(c, rd.data(), 1, r.gamma.data()));
    r.a.assign(m, 0.0);
    for (size_t j = 0; j < m; ++j) r.a[j] = r.gamma[j] * Sd(std::sqrt(r.lambda[j]), zeta[j]);
    std::vector<Real> C(m * m, 0.0);
    if (opt.cqc) check(c, mfh_cqc_matrix((int32_t)m, r.lambda.data(), zeta.data(), C.data()));
    else for (size_t j = 0; j < m; ++j) C[j * m + j] = 1.0;
    for (size_t j = 0; j < m; ++j)
        for (size_t k = 0; k < m; ++k) C[j * m + k] *= r.a[j] * r.a[k];
    const size_t corners = detail::stressCorners(sim);
    r.vonMises.assign(sopt.vonMises ? corners : 0, 0.0);
    r.components.assign(sopt.components ? corners * FL : 0, 0.0);
    check(c, mfh_modal_quadratic_stress(c, 1, C.data(), opt.tol, sopt.flags(), sopt.vonMises ? r.vonMises.data() : nullptr,
                                        sopt.components ? r.components.data() : nullptr, &r.info));
    detail::setStressPeak(r, detail::stressNQ(sim));
    return r;
}

} // namespace MeshFEMHip
