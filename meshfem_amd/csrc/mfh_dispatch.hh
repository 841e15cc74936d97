// Run-time value -> template argument, once for every launcher. A selector hands the functor a std::integral_constant / std::bool_constant
// tag per template parameter; a generic lambda turns the tags into the instantiation and launches it:
//     with_elem(a, [&](auto D, auto G, auto M) { launch_k(k_foo<D(), G(), M()>, grid, block, lds, s, args...); });
// A kernel is instantiated for exactly the tag combinations its selectors can produce. Not part of the ABI.
#pragma once
#include <type_traits>
#include "mfh_internal.hh"

namespace mfh { namespace k {

template <int V> using ic = std::integral_constant<int, V>;

// v among V0, Vs...; a value that is not listed takes the LAST entry (the final else of a ladder)
template <int V0, int... Vs, class F> inline void with_int(int v, F &&f) {
    if constexpr (sizeof...(Vs) == 0) f(ic<V0>{});
    else if (v == V0) f(ic<V0>{});
    else with_int<Vs...>(v, f);
}
template <class F> inline void with_bool(bool b, F &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }

template <class F> inline void with_dim(int dim, F &&f) { with_int<3, 2>(dim, f); }
// kernels with a 1 x 1 (scalar operator) flavour; the digits give the order of the tests: what is neither of the first two takes the third
template <class F> inline void with_dim123(int dim, F &&f) { with_int<3, 2, 1>(dim, f); }
template <class F> inline void with_dim132(int dim, F &&f) { with_int<1, 3, 2>(dim, f); }
template <class F> inline void with_dim_deg(int dim, int deg, F &&f) {
    with_dim(dim, [&](auto D) { with_int<2, 1>(deg, [&](auto G) { f(D, G); }); });
}
// elasticity tensor layout of the geometry records: anything but GENERAL / ORTHO is isotropic
template <class F> inline void with_elasticity(int mat, F &&f) { with_int<MAT_GENERAL, MAT_ORTHO, MAT_ISO>(mat, f); }
// assembly flavours: the elasticity layouts and the scalar operators (LAPLACE unless MASS). Extra...: flavours only some kernels have
// (MAT_MASS_RHO, MAT_GEOM: the gather assembly), taken on an exact match; elsewhere they are scalar operators like any other, i.e. LAPLACE
template <int... Extra, class F> inline void with_asm_flavour(int mat, F &&f) {
    if constexpr (sizeof...(Extra) > 0) {
        if (((mat == Extra) || ...)) { with_int<Extra...>(mat, f); return; }
    }
    if (!mat_is_scalar(mat)) with_elasticity(mat, f);
    else with_int<MAT_MASS, MAT_LAPLACE>(mat, f);
}
// (dim, deg, elasticity layout) / (dim, deg, assembly flavour) of an argument struct with dim, deg, mat
template <class A, class F> inline void with_elem(const A &a, F &&f) {
    with_dim_deg(a.dim, a.deg, [&](auto D, auto G) { with_elasticity(a.mat, [&](auto M) { f(D, G, M); }); });
}
template <int... Extra, class A, class F> inline void with_elem_asm(const A &a, F &&f) {
    with_dim_deg(a.dim, a.deg, [&](auto D, auto G) { with_asm_flavour<Extra...>(a.mat, [&](auto M) { f(D, G, M); }); });
}

// The batch shapes (NR > 1 vectors in lockstep), stated once: f(D, N, NS) = N vectors of dimension D, taken NS at a time (NS is the vector
// stride of the LDS tiles). False, and f not called, for any other pair. op_batch_supported (mfh_kernels.hip) asks select_batch_1d;
// the 1 x 1 shapes exist for the assembled product only.
template <class F> inline bool select_batch(int dim, int nr, F &&f) {
    if (dim == 3 && nr == 2) f(ic<3>{}, ic<2>{}, ic<2>{});
    else if (dim == 3 && nr == 6) f(ic<3>{}, ic<6>{}, ic<2>{});
    else if (dim == 2 && nr == 3) f(ic<2>{}, ic<3>{}, ic<3>{});
    else return false;
    return true;
}
template <class F> inline bool select_batch_1d(int dim, int nr, F &&f) {
    if (dim != 1) return select_batch(dim, nr, f);
    if (nr == 2) f(ic<1>{}, ic<2>{}, ic<2>{});
    else if (nr == 3) f(ic<1>{}, ic<3>{}, ic<3>{});
    else if (nr == 6) f(ic<1>{}, ic<6>{}, ic<3>{});
    else return false;
    return true;
}
// a pair without an instantiation is an error, never a skipped or a mismatched launch
template <class F> inline void with_batch(int dim, int nr, const char *unsupported, F &&f) {
    if (!select_batch(dim, nr, f)) throw Error(MFH_ERR_UNSUPPORTED, unsupported);
}
template <class F> inline void with_batch_1d(int dim, int nr, const char *unsupported, F &&f) {
    if (!select_batch_1d(dim, nr, f)) throw Error(MFH_ERR_UNSUPPORTED, unsupported);
}

// launch one instantiation; more than 64 KB of dynamic LDS has to be granted per function first
template <class K, class... Args> inline void launch_k(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
    if (lds > 64 * 1024) MFH_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}

}} // namespace mfh::k
