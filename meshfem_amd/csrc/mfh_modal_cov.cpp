// Host arithmetic of the random-vibration and response-spectrum layer (mfh_psd_factor, mfh_modal_covariance, mfh_cqc_matrix, include/meshfem_hip.h;
// docs/design/04_23_modal_random.md): no context, no device. Everything the device needs of a spectrum is an nb x nb covariance C of the columns of
// the basis, nb <= 258; the field-sized work is the quadratic form phi_i^T C phi_i per row, which k_modal_sumsq (mfh_modal.hip) evaluates from the
// factor C = F F^T as a sum of squares.
//   mfh_psd_factor        right-looking Cholesky with diagonal pivoting on a symmetric copy W of the lower triangle: at step t the largest remaining
//                         diagonal (the first of equals) is the pivot p; F[:, t] = W[:, p] / sqrt(W[p, p]) on the rows not yet chosen and exactly 0
//                         on the chosen ones; W -= F[:, t] F[:, t]^T, one rounded product and one rounded subtraction per entry. Rows keep their
//                         places (F[j] belongs to column j of the basis); piv lists the pivots.
//   mfh_modal_covariance  C^(p) = sum_k w_k omega_k^p Re(H_k S_k H_k^H), p = 0, 2, 4: every entry is one sum over k in grid order, whatever the
//                         number of host threads (they share the rows of a block of frequencies).
//   mfh_cqc_matrix        Der Kiureghian's correlation with unequal damping, evaluated with r = omega_small / omega_large <= 1 and mirrored.
// The products below are rounded before they are added (no contraction): tests/modal_random_util.py repeats the operations in numpy.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../include/meshfem_hip.h"
#include "mfh_internal.hh"

namespace {

constexpr int COV_MAXB = 258;        // MODAL_MAXB of mfh_modal.hip
constexpr int COV_MAXLOAD = 8;
constexpr int COV_KBLOCK = 64;       // frequencies whose H and H S are formed before the threads add them, in order, to their rows

struct Cx { double re, im; };
inline Cx cmul(const Cx &a, const Cx &b) { return Cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline Cx cinv(const Cx &b) {
    const double d = b.re * b.re + b.im * b.im;
    return Cx{b.re / d, -b.im / d};
}

bool finite_all(const double *v, int64_t count) {
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

}   // namespace

extern "C" {

mfh_status mfh_psd_factor(int32_t n, const double *C, double tol, double *F, int32_t *rank, int32_t *piv, double *truncation) {
    if (rank) *rank = 0;
    if (truncation) *truncation = 0.0;
    if (n < 0 || n > COV_MAXB || (n > 0 && (!C || !F)) || !rank || std::isnan(tol)) return MFH_ERR_INVALID;
    if (n == 0) return MFH_OK;
    std::vector<double> W((size_t)n * n), col((size_t)n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            const double v = C[(size_t)i * n + j];
            if (!std::isfinite(v)) return MFH_ERR_INVALID;
            W[(size_t)i * n + j] = W[(size_t)j * n + i] = v;
        }
    std::fill(F, F + (size_t)n * n, 0.0);
    double dmax = 0.0;
    for (int i = 0; i < n; ++i) dmax = std::max(dmax, W[(size_t)i * n + i]);
    if (tol < 0.0) tol = n * 2.220446049250313e-16 * dmax;
    std::vector<uint8_t> chosen((size_t)n, 0);
    int r = 0;
    for (;; ++r) {
        int p = -1;
        for (int i = 0; i < n; ++i) {
            if (chosen[(size_t)i]) continue;
            const double d = W[(size_t)i * n + i];
            if (d < -tol) return MFH_ERR_INVALID;          // not positive semi-definite
            if (p < 0 || d > W[(size_t)p * n + p]) p = i;
        }
        if (p < 0 || !(W[(size_t)p * n + p] > tol)) break;
        const double l = std::sqrt(W[(size_t)p * n + p]);
        for (int i = 0; i < n; ++i) col[(size_t)i] = chosen[(size_t)i] ? 0.0 : W[(size_t)i * n + p] / l;
        col[(size_t)p] = l;
        for (int i = 0; i < n; ++i) {
            F[(size_t)i * n + r] = col[(size_t)i];
            const double ci = col[(size_t)i];
            double *w = &W[(size_t)i * n];
            for (int j = 0; j < n; ++j) {
                const double prod = ci * col[(size_t)j];
                w[j] = w[j] - prod;
            }
        }
        chosen[(size_t)p] = 1;
        if (piv) piv[r] = p;
    }
    double rest = 0.0;
    for (int i = 0; i < n; ++i)
        if (!chosen[(size_t)i]) rest = rest + std::max(W[(size_t)i * n + i], 0.0);
    if (!std::isfinite(rest) || !finite_all(F, (int64_t)n * n)) return MFH_ERR_INVALID;
    *rank = r;
    if (truncation) *truncation = rest;
    return MFH_OK;
}

mfh_status mfh_cqc_matrix(int32_t m, const double *lambda, const double *zeta, double *rho) {
    if (m < 0 || m > COV_MAXB || (m > 0 && (!lambda || !zeta || !rho))) return MFH_ERR_INVALID;
    for (int j = 0; j < m; ++j)
        if (!std::isfinite(lambda[j]) || !(lambda[j] >= 0.0) || !std::isfinite(zeta[j]) || !(zeta[j] > 0.0)) return MFH_ERR_INVALID;
    for (int j = 0; j < m; ++j) {
        rho[(size_t)j * m + j] = 1.0;
        for (int k = 0; k < j; ++k) {
            // a: the mode of the larger eigenvalue, b: the other; r = omega_b / omega_a <= 1
            const int a = lambda[j] >= lambda[k] ? j : k, b = a == j ? k : j;
            double v = 0.0;
            if (lambda[a] > 0.0) {
                const double r = std::sqrt(lambda[b] / lambda[a]), za = zeta[a], zb = zeta[b], omr2 = (1.0 - r) * (1.0 + r);
                const double num = 8.0 * std::sqrt(za * zb) * (za + r * zb) * r * std::sqrt(r);
                const double den = omr2 * omr2 + 4.0 * za * zb * r * (1.0 + r * r) + 4.0 * (za * za + zb * zb) * r * r;
                v = num / den;
            } else v = zeta[a] == zeta[b] ? 1.0 : 0.0;       // two rigid modes: no oscillation to correlate
            rho[(size_t)j * m + k] = rho[(size_t)k * m + j] = v;
        }
    }
    return MFH_OK;
}

mfh_status mfh_modal_covariance(int32_t m, const double *lambda, const double *g, int32_t nLoad, double rayleighMass, double rayleighStiff, double lossFactor,
                                const double *modalDamping, int32_t nFreq, const double *omega, const double *weights, const double *S, int32_t correction,
                                double *C0, double *C2, double *C4) {
    if (m < 1 || m > COV_MAXB - 2 || nLoad < 1 || nLoad > COV_MAXLOAD || nFreq < 1 || !lambda || !g || !omega || !S || (correction != 0 && correction != 1))
        return MFH_ERR_INVALID;
    if (correction && nLoad > 2) return MFH_ERR_UNSUPPORTED;
    if (!weights && nFreq < 2) return MFH_ERR_INVALID;          // the trapezoid rule needs an interval
    if (!(rayleighMass >= 0.0) || !(rayleighStiff >= 0.0) || !(lossFactor >= 0.0) || !std::isfinite(rayleighMass) || !std::isfinite(rayleighStiff) ||
        !std::isfinite(lossFactor))
        return MFH_ERR_INVALID;
    const int nb = m + (correction ? nLoad : 0), nl = nLoad;
    if (!finite_all(lambda, m) || !finite_all(g, (int64_t)m * nl) || !finite_all(omega, nFreq) || !finite_all(S, (int64_t)nFreq * nl * nl * 2) ||
        (weights && !finite_all(weights, nFreq)) || (modalDamping && !finite_all(modalDamping, m)))
        return MFH_ERR_INVALID;
    bool zeroLambda = false;
    for (int j = 0; j < m; ++j) {
        if (lambda[j] < 0.0 || (modalDamping && modalDamping[j] < 0.0)) return MFH_ERR_INVALID;
        zeroLambda = zeroLambda || lambda[j] == 0.0;
    }
    for (int k = 0; k < nFreq; ++k) {
        if (omega[k] < 0.0 || (k > 0 && !(omega[k] > omega[k - 1]))) return MFH_ERR_INVALID;
        if (omega[k] == 0.0 && zeroLambda) return MFH_ERR_INVALID;
        // S_k Hermitian entry by entry to 8 eps max |S_k|, its diagonal not negative
        const double *Sk = S + (size_t)k * nl * nl * 2;
        double smax = 0.0;
        for (int e = 0; e < nl * nl; ++e) smax = std::max(smax, std::hypot(Sk[2 * e], Sk[2 * e + 1]));
        const double bar = 8.0 * 2.220446049250313e-16 * smax;
        for (int a = 0; a < nl; ++a) {
            if (Sk[(size_t)(a * nl + a) * 2] < 0.0) return MFH_ERR_INVALID;
            for (int b = 0; b <= a; ++b) {
                const double dre = Sk[(size_t)(a * nl + b) * 2] - Sk[(size_t)(b * nl + a) * 2], dim = Sk[(size_t)(a * nl + b) * 2 + 1] + Sk[(size_t)(b * nl + a) * 2 + 1];
                if (std::hypot(dre, dim) > bar) return MFH_ERR_INVALID;
            }
        }
    }
    double *Cp[3] = {C0, C2, C4};
    for (double *c : Cp)
        if (c) std::fill(c, c + (size_t)nb * nb, 0.0);
    // H_k (nb x nLoad) and T_k = H_k S_k of a block of frequencies, then entry (i, j <= i) += w_k omega_k^p Re(sum_b T_ib conj(H_jb)), k ascending
    std::vector<Cx> H((size_t)COV_KBLOCK * nb * nl), T((size_t)COV_KBLOCK * nb * nl);
    std::vector<double> wk((size_t)COV_KBLOCK * 3);
    for (int k0 = 0; k0 < nFreq; k0 += COV_KBLOCK) {
        const int kn = std::min(COV_KBLOCK, nFreq - k0);
        for (int kk = 0; kk < kn; ++kk) {
            const int k = k0 + kk;
            const double w = omega[k];
            const Cx zK{1.0, lossFactor + w * rayleighStiff};
            Cx *h = &H[(size_t)kk * nb * nl], *t = &T[(size_t)kk * nb * nl];
            for (int j = 0; j < m; ++j) {
                const double l = lambda[j];
                const Cx d{l * zK.re - w * w, l * zK.im + w * rayleighMass + (modalDamping ? 2.0 * modalDamping[j] * std::sqrt(l) * w : 0.0)};
                if (d.re == 0.0 && d.im == 0.0) return MFH_ERR_INVALID;
                const Cx di = cinv(d);
                if (!std::isfinite(di.re) || !std::isfinite(di.im)) return MFH_ERR_INVALID;
                for (int a = 0; a < nl; ++a) h[(size_t)j * nl + a] = Cx{g[(size_t)j * nl + a] * di.re, g[(size_t)j * nl + a] * di.im};
            }
            if (correction) {
                const Cx iz = cinv(zK);
                for (int a = 0; a < nl; ++a)
                    for (int b = 0; b < nl; ++b) h[(size_t)(m + a) * nl + b] = a == b ? iz : Cx{0.0, 0.0};
            }
            const double *Sk = S + (size_t)k * nl * nl * 2;
            for (int i = 0; i < nb; ++i)
                for (int b = 0; b < nl; ++b) {
                    Cx acc{0.0, 0.0};
                    for (int a = 0; a < nl; ++a) {
                        const Cx p = cmul(h[(size_t)i * nl + a], Cx{Sk[(size_t)(a * nl + b) * 2], Sk[(size_t)(a * nl + b) * 2 + 1]});
                        acc.re = acc.re + p.re; acc.im = acc.im + p.im;
                    }
                    t[(size_t)i * nl + b] = acc;
                }
            double wq;
            if (weights) wq = weights[k];
            else wq = 0.5 * ((k + 1 < nFreq ? omega[k + 1] : omega[k]) - (k > 0 ? omega[k - 1] : omega[k]));
            const double w2 = w * w;
            wk[(size_t)kk * 3] = wq; wk[(size_t)kk * 3 + 1] = wq * w2; wk[(size_t)kk * 3 + 2] = (wq * w2) * w2;
        }
        mfh::parallel_ranges(nb, [&](int64_t ib, int64_t ie, int) {
            for (int64_t i = ib; i < ie; ++i)
                for (int j = 0; j <= (int)i; ++j)
                    for (int kk = 0; kk < kn; ++kk) {
                        const Cx *t = &T[((size_t)kk * nb + (size_t)i) * nl], *h = &H[((size_t)kk * nb + (size_t)j) * nl];
                        double v = 0.0;
                        for (int b = 0; b < nl; ++b) {
                            const double p1 = t[b].re * h[b].re, p2 = t[b].im * h[b].im;
                            v = v + (p1 + p2);
                        }
                        for (int q = 0; q < 3; ++q)
                            if (Cp[q]) {
                                const double add = wk[(size_t)kk * 3 + q] * v;
                                Cp[q][(size_t)i * nb + j] = Cp[q][(size_t)i * nb + j] + add;
                            }
                    }
        }, 16);
    }
    for (double *c : Cp)
        if (c) {
            for (int i = 0; i < nb; ++i)
                for (int j = 0; j < i; ++j) c[(size_t)j * nb + i] = c[(size_t)i * nb + j];
            if (!finite_all(c, (int64_t)nb * nb)) return MFH_ERR_INVALID;
        }
    return MFH_OK;
}

}   // extern "C"
