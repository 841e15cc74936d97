// Stress measures on the MI355X path: the facade of the reference's VonMises.hh (vonMises) and of SymmetricMatrix.hh's eigenvalues /
// eigenDecomposition over the C ABI (include/meshfem_hip.h, "stress measures on the device").
//   vonMises(simOrCtx, field) / vonMises(field)      the von Mises SCALAR of every flattened symmetric matrix of `field`: the Frobenius norm of
//                                                    the reference's vonMises(field)(i) = vonMisesExtractor<N>().doubleContract(field(i))
//                                                    (VonMises.hh:100-107), which is the number its callers take from that tensor
//   eigenvalues(simOrCtx, field)                     ascending, N per matrix (SymmetricMatrix.hh eigenvalues)
//   eigenDecomposition(simOrCtx, field)              {eigenvalues, eigenvectors}: N x N per matrix, row-major, eigenvector k in column k
//   vonMisesStress / principalStresses(sim, uNodes)  the same measures of the stress (stress = false: strain) of a displacement field at the
//                                                    corners of Simulator::stressField, fused on the device: the tensor is never stored
//   peakVonMises(sim, uNodes)                        {max von Mises value over all corners, flat corner index}; nothing but two numbers
//                                                    leaves the device
// Fields are std::vector<std::array<Real, flatLen>> (Simulator::SMField; tensor shear entries). simOrCtx is a Simulator (anything with
// ctx()) or a raw mfh_ctx*; the one-argument forms run on a context of their own on device 0.
#pragma once

#include <utility>

#include "LinearElasticity.hh"

namespace MeshFEMHip {
namespace detail {

inline mfh_ctx *ctxOf(mfh_ctx *c) { return c; }
template <class Sim> mfh_ctx *ctxOf(const Sim &sim) { return sim.ctx(); }

template <size_t FL> struct DimOfFlatLen;
template <> struct DimOfFlatLen<3> { static constexpr size_t value = 2; };
template <> struct DimOfFlatLen<6> { static constexpr size_t value = 3; };

// a context that needs no mesh: device and stream only
struct ScratchContext {
    mfh_ctx *c = nullptr;
    explicit ScratchContext(int device) {
        if (mfh_create(device, &c) != MFH_OK) throw std::runtime_error("mfh_create failed: no usable HIP device (there is no CPU fallback)");
    }
    ~ScratchContext() { if (c) mfh_destroy(c); }
    ScratchContext(const ScratchContext &) = delete;
    ScratchContext &operator=(const ScratchContext &) = delete;
};

template <size_t FL>
void symMeasures(mfh_ctx *c, const std::vector<std::array<Real, FL>> &field, int32_t what, std::vector<Real> *vm, std::vector<Real> *eval,
                 std::vector<Real> *evec) {
    constexpr size_t N = DimOfFlatLen<FL>::value;
    const size_t n = field.size();
    if (vm) vm->resize(n);
    if (eval) eval->resize(n * N);
    if (evec) evec->resize(n * N * N);
    if (n == 0) return;
    check(c, mfh_sym_measures(c, (int32_t)N, (int64_t)n, &field[0][0], what, vm ? vm->data() : nullptr, eval ? eval->data() : nullptr,
                              evec ? evec->data() : nullptr, 0));
}

template <class Sim> size_t cornerCount(const Sim &sim) {
    int64_t nElem = 0;
    int32_t npe = 0;
    check(sim.ctx(), mfh_mesh_sizes(sim.ctx(), &nElem, nullptr, nullptr, nullptr, nullptr, &npe, nullptr));
    return (size_t)nElem * (npe == 3 || npe == 4 ? 1 : (npe == 6 ? 3 : 4));
}

} // namespace detail

template <class SimOrCtx, size_t FL> std::vector<Real> vonMises(const SimOrCtx &simOrCtx, const std::vector<std::array<Real, FL>> &field) {
    std::vector<Real> vm;
    detail::symMeasures(detail::ctxOf(simOrCtx), field, MFH_MEASURE_VON_MISES, &vm, nullptr, nullptr);
    return vm;
}
template <size_t FL> std::vector<Real> vonMises(const std::vector<std::array<Real, FL>> &field) {
    detail::ScratchContext s(0);
    return vonMises(s.c, field);
}

template <class SimOrCtx, size_t FL> std::vector<Real> eigenvalues(const SimOrCtx &simOrCtx, const std::vector<std::array<Real, FL>> &field) {
    std::vector<Real> ev;
    detail::symMeasures(detail::ctxOf(simOrCtx), field, MFH_MEASURE_EIGENVALUES, nullptr, &ev, nullptr);
    return ev;
}
template <size_t FL> std::vector<Real> eigenvalues(const std::vector<std::array<Real, FL>> &field) {
    detail::ScratchContext s(0);
    return eigenvalues(s.c, field);
}

template <class SimOrCtx, size_t FL>
std::pair<std::vector<Real>, std::vector<Real>> eigenDecomposition(const SimOrCtx &simOrCtx, const std::vector<std::array<Real, FL>> &field) {
    std::pair<std::vector<Real>, std::vector<Real>> r;
    detail::symMeasures(detail::ctxOf(simOrCtx), field, MFH_MEASURE_EIGENVALUES | MFH_MEASURE_EIGENVECTORS, nullptr, &r.first, &r.second);
    return r;
}

// [nElem][1 | N+1] von Mises values of the stress (strain) of uNodes
template <class Sim> std::vector<Real> vonMisesStress(const Sim &sim, const typename Sim::VField &uNodes, bool stress = true) {
    std::vector<Real> vm(detail::cornerCount(sim));
    check(sim.ctx(), mfh_stress_measures(sim.ctx(), &uNodes[0][0], stress ? 1 : 0, MFH_MEASURE_VON_MISES, vm.data(), nullptr, nullptr, 0));
    return vm;
}

// [nElem][1 | N+1][N] ascending principal stresses (strains) of uNodes
template <class Sim> std::vector<Real> principalStresses(const Sim &sim, const typename Sim::VField &uNodes, bool stress = true) {
    constexpr size_t N = std::tuple_size<typename Sim::VField::value_type>::value;
    std::vector<Real> ev(detail::cornerCount(sim) * N);
    check(sim.ctx(), mfh_stress_measures(sim.ctx(), &uNodes[0][0], stress ? 1 : 0, MFH_MEASURE_EIGENVALUES, nullptr, ev.data(), nullptr, 0));
    return ev;
}

template <class Sim> std::pair<Real, int64_t> peakVonMises(const Sim &sim, const typename Sim::VField &uNodes, bool stress = true) {
    std::pair<Real, int64_t> r{0.0, -1};
    check(sim.ctx(), mfh_peak_von_mises(sim.ctx(), &uNodes[0][0], stress ? 1 : 0, &r.first, &r.second));
    return r;
}

} // namespace MeshFEMHip
