"""The list-mode transform restated independently of chronoclust_amd: compensation as an explicit loop over j with
elementwise numpy operations only (never `x @ M`: BLAS fuses and reorders), the variants a test tells it apart from (every step
fused, computed exactly with fractions.Fraction; descending j), arcsinh through extended precision, distances in units in the
last place, and the inputs - record buffers, spillover matrices and their inverses - the tests of the `_list_xf` route share."""
from fractions import Fraction

import numpy as np

import fcs_util as F

LITTLE, BIG = (1, 2, 3, 4), (4, 3, 2, 1)


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float64
    return a.view(np.int64)


def same_bits(got, exp, what):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape, "%s: shapes %r / %r" % (what, got.shape, exp.shape)
    ne = np.argwhere(bits(got) != bits(exp))
    assert ne.size == 0, "%s: %d of %d differ, first at %r: %r / %r" % (what, len(ne), got.size, tuple(ne[0]), got[tuple(ne[0])],
                                                                      exp[tuple(ne[0])])


def decoded(rec, cols, masks=None):
    """float64 of the selected columns of native records, integers under their masks."""
    out = rec[:, cols]
    if masks is not None:
        out = out & np.asarray(masks, np.uint32).astype(rec.dtype)
    return np.ascontiguousarray(out.astype(np.float64))


def comp_inputs(rec, cols, masks, comp_cols):
    """float64 [n, m] of the compensated columns: each under the mask of the first selected dimension that names it."""
    cols = [int(c) for c in cols]
    xs = np.empty((rec.shape[0], len(comp_cols)), np.float64)
    for j, c in enumerate(comp_cols):
        x = rec[:, int(c)]
        if masks is not None and int(c) in cols:
            x = x & np.uint32(masks[cols.index(int(c))]).astype(rec.dtype)
        xs[:, j] = x.astype(np.float64)
    return xs


def compensated(x, xs, cols, comp_cols, comp, descending=False):
    """The specification: for a selected dimension whose source column is comp_cols[i],
    v = ((xs[0] * comp[0][i]) + xs[1] * comp[1][i]) + ... in ascending j, each product and each sum rounded to double;
    every other dimension keeps x.  descending: the same sum from the other end (what a test tells apart)."""
    out = np.array(x, dtype=np.float64, copy=True)
    comp_cols = [int(c) for c in comp_cols]
    m = len(comp_cols)
    order = list(range(m))[::-1] if descending else list(range(m))
    for k, c in enumerate(int(c) for c in cols):
        if c not in comp_cols:
            continue
        i = comp_cols.index(c)
        acc = None
        for j in order:
            prod = np.multiply(xs[:, j], comp[j][i])
            acc = prod if acc is None else np.add(acc, prod)
        out[:, k] = acc
    return out


def _fma(a, b, c):
    """round(a * b + c), exactly: one rounding"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def compensated_fused(x, xs, cols, comp_cols, comp):
    """The same sum with every step fused (v = fma(x_j, comp_ji, v)), exact through fractions.Fraction: what a build that
    contracts would compute."""
    out = np.array(x, dtype=np.float64, copy=True)
    comp_cols = [int(c) for c in comp_cols]
    for k, c in enumerate(int(c) for c in cols):
        if c not in comp_cols:
            continue
        i = comp_cols.index(c)
        for r in range(len(out)):
            acc = float(xs[r, 0]) * float(comp[0][i])
            for j in range(1, len(comp_cols)):
                acc = _fma(float(xs[r, j]), float(comp[j][i]), acc)
            out[r, k] = acc
    return out


def asinh_reference(q):
    """arcsinh correctly rounded but for the reference's own last rounding: through extended precision where numpy has it."""
    q = np.asarray(q, np.float64)
    if np.finfo(np.longdouble).nmant >= 63:
        return np.arcsinh(q.astype(np.longdouble)).astype(np.float64)
    return np.arcsinh(q)


def with_cofactors(v, cofactor):
    """v [n, d] after the cofactors: asinh_reference(v / c) where c > 0, v where c == 0."""
    out = np.array(v, dtype=np.float64, copy=True)
    for k, c in enumerate(np.asarray(cofactor, np.float64).tolist()):
        if c > 0:
            out[:, k] = asinh_reference(np.divide(v[:, k], c))
    return out


def ulp_distance(a, b):
    """Units in the last place between float64 arrays of finite values (the integers of their ordered bit patterns)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    return np.abs(ordered(a) - ordered(b))


def spillover(m, seed):
    """(spillover matrix, its inverse) [m, m]: unit diagonal, neighbours spilling 2 .. 25 %, a few per cent further out."""
    rng = np.random.default_rng(seed)
    s = np.eye(m)
    for i in range(m):
        for j in range(m):
            if i != j:
                s[i, j] = rng.uniform(0.02, 0.25) if abs(i - j) <= 2 else rng.uniform(0.0, 0.02)
    inv = np.linalg.inv(s)
    assert np.isfinite(inv).all()
    return s, np.ascontiguousarray(inv)


def records(dtype, n, src_cols, seed, top=2.0 ** 18):
    """Native [n, src_cols]: values up to `top` for the floating types (some negative: compensated events are), the whole
    range for integers."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype.kind == "f":
        rec = (rng.uniform(-0.02, 1.0, (n, src_cols)) ** 3 * top).astype(dtype)
    else:
        rec = rng.integers(0, np.iinfo(dtype).max, (n, src_cols), dtype=dtype, endpoint=True)
    return rec


def list_mode(rec, order, cols=None, masks=None, transform=None):
    """The ListMode of native records `rec`, written in byte order `order`, one byte past an aligned address."""
    from chronoclust_amd import _lib
    buf = F.unaligned(F.fast_records(rec, order))
    dt = rec.dtype.newbyteorder("<" if order == LITTLE else ">") if rec.dtype.itemsize > 1 else rec.dtype
    lm = _lib.ListMode(buf, rec.shape[0], rec.shape[1], dt, columns=cols, masks=masks, transform=transform)
    assert lm._bytes.ctypes.data % 64 == 1 or rec.size == 0
    return lm


def spillover_text(names, spill):
    """The value of a $SPILLOVER keyword: n, the names, the n * n values row-major (repr: every double survives)."""
    return ",".join([str(len(names))] + list(names) + [repr(float(v)) for v in np.asarray(spill).ravel()])
