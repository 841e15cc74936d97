// The eight coefficients of the exact step of one mode under a piecewise-linear load (mfh_modal_transient_coeffs, include/meshfem_hip.h;
// docs/design/04_22_modal_transient.md): host only, no context, no device.
//     q'' + c q' + lambda q = a(t),  a linear over the step:   [q ; q']_{n+1} = A [q ; q']_n + b0 a_n + b1 (a_{n+1} - a_n) / dt
// With S the impulse response (S(0) = 0, S'(0) = 1), I0 = int_0^t S and I1 = int_0^t I0, all taken at t = dt:
//     A = [[S' + c S, S], [-lambda S, S']],   b0 = [I0 ; S],   b1 = [I1 ; I0].
// The textbook closed forms lose everything to cancellation for small omega dt, and give NaN for lambda = 0 and for c^2 > 4 lambda. Here the four
// functions are formed in long double in one of three regimes, none of which subtracts nearly equal numbers beyond a few bits, and rounded to double:
//   series     dt max(sqrt(lambda), c) <= 1: the Taylor series through the recurrence s_{k+2} = -c s_{k+1} - lambda s_k of the derivatives of S at 0,
//              in the scaled terms sigma_k = s_k dt^(k-1) (|sigma_k| <= 1.62^k, so forty terms of sigma_k / k! end below 1e-30);
//   roots      over-damped with well separated real roots r1 = -lambda / (alpha + mu) (slow), r2 = -(alpha + mu) (fast), alpha = c / 2,
//              mu = sqrt(alpha^2 - lambda) >= alpha / 4: divided differences of e^x, (e^x - 1) / x and (e^x - 1 - x) / x^2 at x = r dt. lambda = 0 with
//              c > 0 is this regime with r1 = 0;
//   envelope   everything else (under-damped, critical, nearly critical on either side): e^(-alpha dt) times cos / sinc or cosh / sinhc of mu dt, and
//              I0 = (1 - A11) / lambda, I1 = (dt - c I0 - S) / lambda, which is safe here because lambda >= (15/16) alpha^2 and dt sqrt(lambda) > 1/2.
#include <cmath>
#include "../../include/meshfem_hip.h"

namespace {

typedef long double ld;

// (e^x - 1) / x
ld phi1(ld x) { return x == 0.0L ? 1.0L : expm1l(x) / x; }
// (e^x - 1 - x) / x^2 for x <= 0
ld phi2(ld x) {
    if (x > -1.0L) {
        ld term = 0.5L, sum = 0.5L;
        for (int k = 1; k < 40; ++k) { term *= x / (ld)(k + 2); sum += term; }
        return sum;
    }
    return (expm1l(x) - x) / (x * x);
}

struct Four { ld S, dS, I0, I1, A11; };

Four series(ld lam, ld c, ld t) {
    // sigma_k = s_k t^(k-1): sigma_0 = 0, sigma_1 = 1, sigma_{k+2} = -(c t) sigma_{k+1} - (lambda t^2) sigma_k
    const ld ct = c * t, lt2 = lam * t * t;
    ld s0 = 0.0L, s1 = 1.0L;          // sigma_k, sigma_{k+1}
    ld fk = 1.0L;                     // 1 / k!
    ld S = 0.0L, dS = 0.0L, I0 = 0.0L, I1 = 0.0L;
    for (int k = 0; k < 40; ++k) {
        if (k > 0) fk /= (ld)k;
        S += s0 * fk;                                   // S / t        = sum sigma_k / k!           (t^k s_k = t sigma_k)
        dS += s1 * fk;                                  // S'           = sum sigma_{k+1} / k!
        I0 += s0 * fk / (ld)(k + 1);                    // I0 / t^2     = sum sigma_k / (k+1)!
        I1 += s0 * fk / ((ld)(k + 1) * (ld)(k + 2));    // I1 / t^3     = sum sigma_k / (k+2)!
        const ld s2 = -ct * s1 - lt2 * s0;
        s0 = s1; s1 = s2;
    }
    Four f;
    f.S = S * t; f.dS = dS; f.I0 = I0 * t * t; f.I1 = I1 * t * t * t;
    f.A11 = 1.0L - lam * f.I0;        // (S' + c S + lambda I0 = 1; lambda I0 <= 1/2 here)
    return f;
}

Four roots(ld lam, ld alpha, ld mu, ld t) {
    const ld r2 = -(alpha + mu), r1 = -lam / (alpha + mu), x1 = r1 * t, x2 = r2 * t, e1 = expl(x1), e2 = expl(x2), d = 2.0L * mu;
    Four f;
    f.S = (e1 - e2) / d;
    f.dS = (r1 * e1 - r2 * e2) / d;
    f.A11 = (r1 * e2 - r2 * e1) / d;
    f.I0 = t * (phi1(x1) - phi1(x2)) / d;
    f.I1 = t * t * (phi2(x1) - phi2(x2)) / d;
    return f;
}

Four envelope(ld lam, ld c, ld alpha, ld D, ld t) {
    const ld at = alpha * t;
    ld ch, sc;        // e^(-alpha t) cos|cosh(mu t),  e^(-alpha t) sin|sinh(mu t) / (mu t)
    if (D < 0.0L) {
        const ld y = sqrtl(-D) * t, e = expl(-at);
        ch = e * cosl(y);
        sc = e * (y == 0.0L ? 1.0L : sinl(y) / y);
    } else {
        const ld y = sqrtl(D) * t, e = expl(y - at), em = expl(-2.0L * y);       // (y <= alpha t / 4: e does not overflow)
        ch = e * (1.0L + em) * 0.5L;
        sc = y == 0.0L ? e : e * (-expm1l(-2.0L * y)) / (2.0L * y);
    }
    Four f;
    f.S = t * sc;
    f.dS = ch - at * sc;
    f.A11 = ch + at * sc;
    f.I0 = (1.0L - f.A11) / lam;
    f.I1 = (t - c * f.I0 - f.S) / lam;
    return f;
}

}   // namespace

extern "C" mfh_status mfh_modal_transient_coeffs(double lambda, double c, double dt, double *out8) {
    if (!out8 || !(lambda >= 0.0) || !(c >= 0.0) || !(dt > 0.0) || !std::isfinite(lambda) || !std::isfinite(c) || !std::isfinite(dt)) return MFH_ERR_INVALID;
    const ld lam = lambda, cc = c, t = dt, alpha = 0.5L * cc;
    const ld D = fmal(alpha, alpha, -lam);          // alpha^2 - lambda, rounded once
    Four f;
    if (t * fmaxl(sqrtl(lam), cc) <= 1.0L) f = series(lam, cc, t);
    else if (D > 0.0L && sqrtl(D) >= 0.25L * alpha) f = roots(lam, alpha, sqrtl(D), t);
    else f = envelope(lam, cc, alpha, D, t);
    out8[0] = (double)f.A11; out8[1] = (double)f.S; out8[2] = (double)f.I0; out8[3] = (double)f.I1;
    out8[4] = (double)(-lam * f.S); out8[5] = (double)f.dS; out8[6] = (double)f.S; out8[7] = (double)f.I0;
    return MFH_OK;
}
