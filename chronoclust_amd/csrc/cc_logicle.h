// cc_logicle.h — the coefficients of the logicle (biexponential) display scale of Parks, Roederer and Moore 2006 in the
// parameterisation of Moore and Parks 2012 (T, W, M, A), derived ONCE per dimension on the host: cc_logicle_derive is the one
// place where they are computed - cc_logicle_coefficients hands them out, list_check_lg (cc_api_list.inc) lays them behind the
// transform in the device buffer and cc_logicle_value (cc_ingest_list_xf.h) solves with them.
//   w = W / (M + A)   x2 = A / (M + A)   x1 = x2 + w   x0 = x2 + 2 w   b = (M + A) ln 10
//   d: the root in (0, b] of 2 (ln d - ln b) + w (d + b) = 0 (w == 0: d = b)
//   ca = exp(x0 (b + d))   mf = exp(b x1) - ca exp(-d x1)   a = T / ((exp(b) - mf) - ca exp(-d))
//   pa = a exp(b x1)       pc = a ca exp(-d x1)
//   G(u) = pa (exp(b u) - 1) - pc (exp(-d u) - 1), u >= 0: G(0) = 0, G(1 - x1) = T, G''(0) = 0, G' > 0
//   logicle(v) = x1 + sign(v) u with G(u) = |v|: the unit display scale - T maps to 1, 0 to x1; nothing is clipped
// w, x2, x1 and x0 are the doubles of the formulas above (x1 is what logicle(0) returns, and every later quantity is derived
// from THAT x1, so G(1 - x1) = T holds for the x1 the kernels add); everything behind them is computed in long double and
// rounded once.  Plain host code: no handle, no HIP.
#pragma once

#include <cmath>

namespace {

// out = {x1, b, d, pa, pc, 0, 0, 0}; a row with T == 0 is off the scale: all zeros (pa == 0 is what switches the solve off).
// Returns null, or the reason the parameters are refused for.
inline const char* cc_logicle_derive(const double twma[4], double out[8])
{
    for (int i = 0; i < 8; ++i) out[i] = 0.0;
    const double T = twma[0], W = twma[1], M = twma[2], A = twma[3];
    if (!std::isfinite(T) || !std::isfinite(W) || !std::isfinite(M) || !std::isfinite(A)) return "a parameter is not finite";
    if (T < 0.0) return "T is negative";
    if (T == 0.0) return nullptr;
    if (M <= 0.0) return "M must be positive";
    if (W < 0.0) return "W is negative";
    if (2.0 * W > M) return "2 W exceeds M";
    if (A < -W) return "A is below -W";
    if (A > M - 2.0 * W) return "A exceeds M - 2 W";
    const double s = M + A;
    if (!(s > 0.0) || !std::isfinite(s)) return "M + A must be positive";
    const double w = W / s, x2 = A / s, x1 = x2 + w, x0 = x2 + 2.0 * w;
    const long double b = ((long double)M + (long double)A) * logl(10.0L);
    long double d = b;
    if (w > 0.0) {
        // h(d) = 2 (ln d - ln b) + w (d + b) rises from -inf at 0 to 2 w b at b: bisection to the last bit
        const long double lb = logl(b);
        long double lo = 0.0L, hi = b;
        for (int i = 0; i < 20000; ++i) {
            const long double mid = 0.5L * (lo + hi);
            if (mid == lo || mid == hi) break;
            if (2.0L * (logl(mid) - lb) + (long double)w * (mid + b) < 0.0L) lo = mid;
            else hi = mid;
        }
        d = hi;
    }
    const long double ca = expl((long double)x0 * (b + d));
    const long double mf = expl(b * x1) - ca * expl(-d * x1);
    const long double a = (long double)T / ((expl(b) - mf) - ca * expl(-d));
    out[0] = x1;
    out[1] = (double)b;
    out[2] = (double)d;
    out[3] = (double)(a * expl(b * x1));
    out[4] = (double)(a * ca * expl(-d * x1));
    for (int i = 0; i < 5; ++i)
        if (!std::isfinite(out[i])) return "the coefficients overflow a double";
    if (!(out[2] > 0.0) || !(out[3] > 0.0) || !(out[4] > 0.0)) return "the coefficients underflow a double";
    return nullptr;
}

}  // namespace
