// Per-element density and the mass of the body on the MI355X path, over the C ABI (include/meshfem_hip.h, "per-element density"). The reference has no
// counterpart: its mass matrices are at unit density.
//   setDensity(sim, rho)          the density field of the mass matrix of vibrationalModes (Eigensolver.hh) and transient (Dynamics.hh): one strictly
//                                 positive value per element; an empty vector restores unit density. Their scalar density multiplies the field.
//   massProperties(sim, scale)    {mass, com, secondMoment S = int rho (x - com)(x - com)^T, inertia = tr(S) I - S about the centre of mass (the tensor
//                                 of a 3D body), polar = tr(S) (the polar moment of a 2D body)} under the field times the scalar scale
//   applyMass(sim, x)             M x for one N-vector per DoF: the consistent mass matrix with the density field, no variables masked
//   lumpedMassHRZ(sim)            the HRZ-lumped masses (diagonal of the element mass matrices scaled to the element's mass), one N-vector per DoF
// Each throws std::runtime_error where the C call fails.
#pragma once

#include <array>

#include "LinearElasticity.hh"

namespace MeshFEMHip {

template <size_t N>
struct MassPropertiesResult {
    Real mass = 0.0;
    std::array<Real, N> com{};
    std::array<std::array<Real, N>, N> secondMoment{}, inertia{};   // inertia: tr(S) I - S (the tensor of a 3D body about its centre of mass)
    Real polar = 0.0;                                              // tr(S): the polar moment of a 2D body
};

template <class Sim>
void setDensity(const Sim &sim, const std::vector<Real> &rho) {
    mfh_ctx *c = sim.ctx();
    check(c, mfh_set_density(c, rho.empty() ? nullptr : rho.data(), (int64_t)rho.size(), 0));
}

template <class Sim>
MassPropertiesResult<std::tuple_size<typename Sim::VField::value_type>::value> massProperties(const Sim &sim, Real scale = 1.0) {
    constexpr size_t N = std::tuple_size<typename Sim::VField::value_type>::value;
    mfh_ctx *c = sim.ctx();
    MassPropertiesResult<N> r;
    Real S[N * N];
    check(c, mfh_mass_properties(c, scale, &r.mass, r.com.data(), S, 0));
    for (size_t a = 0; a < N; ++a) r.polar += S[a * N + a];
    for (size_t a = 0; a < N; ++a)
        for (size_t b = 0; b < N; ++b) {
            r.secondMoment[a][b] = S[a * N + b];
            r.inertia[a][b] = (a == b ? r.polar : 0.0) - S[a * N + b];
        }
    return r;
}

template <class Sim>
typename Sim::VField applyMass(const Sim &sim, const typename Sim::VField &x) {
    mfh_ctx *c = sim.ctx();
    if (x.size() != sim.numDoFs()) throw std::runtime_error("applyMass: x needs one entry per DoF");
    typename Sim::VField y(x.size());
    check(c, mfh_mass_apply(c, &x[0][0], &y[0][0], 0));
    return y;
}

// The HRZ-lumped masses, one N-vector per DoF (the mass of a DoF repeated for its components): positive on linear and quadratic elements alike,
// the density field inside; the mass matrix of explicitTransient (Dynamics.hh).
template <class Sim>
typename Sim::VField lumpedMassHRZ(const Sim &sim) {
    mfh_ctx *c = sim.ctx();
    typename Sim::VField m(sim.numDoFs());
    check(c, mfh_mass_lumped_hrz(c, &m[0][0], 0));
    return m;
}

} // namespace MeshFEMHip
