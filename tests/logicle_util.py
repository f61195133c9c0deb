"""The logicle (biexponential) display scale of Parks, Roederer and Moore 2006 in the parameterisation of Moore and Parks 2012
(T, W, M, A), restated independently of chronoclust_amd: the referee of the `_list_xl` route.  The coefficients are derived
from T, W, M, A alone in np.longdouble - d by bisection to the last bit -, the root of G(u) = |v| by Newton from above (G is
increasing and convex for u >= 0, so the iterates fall monotonically onto the root) with expm1 in np.longdouble, to a fixed
point, and the result is rounded ONCE to float64.  Distances are counted in units of np.spacing(max(|y_ref|, 0.5)): the result
is a display coordinate that crosses zero, so relative units in the last place of y mean nothing there.
    w = W / (M + A)   x2 = A / (M + A)   x1 = x2 + w   x0 = x2 + 2 w   b = (M + A) ln 10
    d: 2 (ln d - ln b) + w (d + b) = 0 in (0, b]       ca = exp(x0 (b + d))       mf = exp(b x1) - ca exp(-d x1)
    a = T / ((exp(b) - mf) - ca exp(-d))               pa = a exp(b x1)           pc = a ca exp(-d x1)
    G(u) = pa (exp(b u) - 1) - pc (exp(-d u) - 1);     logicle(v) = x1 + sign(v) u,  G(u) = |v|"""
import numpy as np

LD = np.longdouble
EXTENDED = np.finfo(LD).nmant >= 63
NEEDS_EXTENDED = "np.longdouble is no wider than float64 here: the referee is no better than what it referees"

# (T, W, M, A): the common flow setting, a shifted one, a narrow one, w = 0 (d = b), a wide one, A = -W, A = M - 2 W, 2 W = M
P = [(262144.0, 0.5, 4.5, 0.0), (262144.0, 1.0, 4.5, 0.5), (10000.0, 0.25, 4.0, 0.0), (262144.0, 0.0, 4.5, 0.0),
     (4194304.0, 2.0, 5.5, 1.0), (1000.0, 0.5, 4.5, -0.5), (262144.0, 1.0, 4.5, 2.5), (262144.0, 2.25, 4.5, 0.0)]


def coefficients(T, W, M, A, real=LD, log=np.log, exp=np.exp):
    """dict of w, x1, b, d, pa, pc in `real` arithmetic (np.longdouble; mpmath.mpf with its log and exp for the 40-digit
    check)."""
    T, W, M, A = (real(float(v)) for v in (T, W, M, A))  # (exact: a double is one in either arithmetic)
    w = W / (M + A)
    x2 = A / (M + A)
    x1 = x2 + w
    x0 = x2 + 2 * w
    b = (M + A) * log(real(10))
    if w == 0:
        d = b
    else:
        lo, hi = b * 0, b  # h(lo) < 0 <= h(hi), h increasing
        for _ in range(400):
            mid = (lo + hi) / 2
            if mid == lo or mid == hi:
                break
            if 2 * (log(mid) - log(b)) + w * (mid + b) < 0:
                lo = mid
            else:
                hi = mid
        d = hi
    ca = exp(x0 * (b + d))
    mf = exp(b * x1) - ca * exp(-d * x1)
    a = T / ((exp(b) - mf) - ca * exp(-d))
    return dict(w=w, x1=x1, b=b, d=d, pa=a * exp(b * x1), pc=a * ca * exp(-d * x1))


def G(c, u, expm1=np.expm1):
    return c["pa"] * expm1(c["b"] * u) - c["pc"] * expm1(-c["d"] * u)


def logicle(v, T, W, M, A):
    """The referee: logicle(v) for a float64 array of finite values, in np.longdouble, rounded once to float64."""
    c = coefficients(T, W, M, A)
    v = np.asarray(v, np.float64)
    y = np.abs(v).astype(LD)
    pa, pc, b, d = c["pa"], c["pc"], c["b"], c["d"]
    with np.errstate(all="ignore"):
        # both starts lie at or above the root: G(u) >= G'(0) u (convex) and G(u) >= pa (exp(b u) - 1)
        u = np.minimum(y / (pa * b + pc * d), np.log1p(y / pa) / b)
        for _ in range(300):
            e1, e2 = np.expm1(b * u), np.expm1(-d * u)
            f = pa * e1 - pc * e2 - y
            nxt = u - f / (pa * b * (e1 + 1) + pc * d * (e2 + 1))
            nxt = np.where(nxt < u, nxt, u)  # (from above: an iterate that does not fall has arrived)
            nxt = np.where(nxt > 0, nxt, u * 0)
            if (nxt == u).all():
                break
            u = nxt
        else:
            raise AssertionError("the referee's Newton iteration did not settle")
    return (c["x1"] + np.where(np.signbit(v), -u, u)).astype(np.float64)


def inverse(y, T, W, M, A):
    """The values whose logicle is (about) y: sign(y - x1) G(|y - x1|), in np.longdouble, rounded to float64.  For building
    inputs: any rounding will do."""
    c = coefficients(T, W, M, A)
    t = np.asarray(y, np.float64).astype(LD) - c["x1"]
    return (np.sign(t) * G(c, np.abs(t))).astype(np.float64)


def units(y, y_ref):
    """The distance of y from y_ref in units of np.spacing(max(|y_ref|, 0.5))."""
    y, y_ref = np.asarray(y, np.float64), np.asarray(y_ref, np.float64)
    return np.abs(y - y_ref) / np.spacing(np.maximum(np.abs(y_ref), 0.5))


def sweep_bands(T):
    """[(lo, hi)] of |v|: three decades each from 1e-6 on, the last one ending at 2 T."""
    out, lo = [], 1e-6
    while lo * 1000.0 < 2 * T:
        out.append((lo, lo * 1000.0))
        lo *= 1000.0
    out.append((lo, 2 * T))
    return out


def sweep(T, per_band=20000, seed=3):
    """|v| log-uniform per band of sweep_bands(T), per_band values each, both signs; then +0.0, -0.0, T, -T, the smallest
    subnormal and 1e300: a flat float64 array whose length is a multiple of 4."""
    rng = np.random.default_rng(seed)
    mags = [np.exp(rng.uniform(np.log(lo), np.log(hi), per_band)) for lo, hi in sweep_bands(T)]
    mags[-1][0], mags[0][0] = 2 * T, 1e-6  # (both ends of the range are reached)
    v = np.concatenate(mags)
    v = np.concatenate([v, -v, [0.0, -0.0, T, -T, 5e-324, 1e300]])
    return np.concatenate([v, np.full(-len(v) % 4, 1.0)])


_MP_COEFFICIENTS = {}


def mp_logicle(v, T, W, M, A, digits=40):
    """logicle(v) of one finite float by a 40-digit evaluation (mpmath), as an mpf."""
    import mpmath
    with mpmath.workdps(digits):
        mpf = mpmath.mpf
        key = (T, W, M, A, digits)
        if key not in _MP_COEFFICIENTS:
            _MP_COEFFICIENTS[key] = coefficients(T, W, M, A, real=mpf, log=mpmath.log, exp=mpmath.exp)
        c = _MP_COEFFICIENTS[key]
        y = abs(mpf(float(v)))
        u = min(y / (c["pa"] * c["b"] + c["pc"] * c["d"]), mpmath.log1p(y / c["pa"]) / c["b"])
        for _ in range(500):
            e1, e2 = mpmath.expm1(c["b"] * u), mpmath.expm1(-c["d"] * u)
            f = c["pa"] * e1 - c["pc"] * e2 - y
            step = f / (c["pa"] * c["b"] * (e1 + 1) + c["pc"] * c["d"] * (e2 + 1))
            u -= step
            if abs(step) <= abs(u) * mpf(10) ** (3 - digits):
                break
        return c["x1"] + (-u if v < 0 or (v == 0 and np.signbit(v)) else u)
