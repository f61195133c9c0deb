"""The referee of the negative quantiles (cc_negq_*, Handle.negative_quantiles, fcs.estimate_logicle) and the inputs its tests
share.  The referee restates the contract from numpy alone: np.asarray of every source with its compensation only (the device's
left-to-right sum, bit for bit), neg = v[v < 0] pooled, np.sort, the indices of numpy's linear method, np.quantile(neg, q), and
the width formula written out.  It calls nothing of the code under test but ListMode's host decode."""
import numpy as np

import transform_util as U

LITTLE, BIG = U.LITTLE, U.BIG
QS = (0.0, 0.05, 0.25, 0.5, 1.0)
# the selection's own partition (csrc/cc_negq.h): elements of a column per workgroup, threads per workgroup, lanes per wave
NEGQ_CHUNK = 8192
NEGQ_THREADS = 256
WAVE = 64
SEAM_NS = sorted(set(n for edge in (WAVE, NEGQ_THREADS, NEGQ_CHUNK, 2 * NEGQ_CHUNK, 12 * NEGQ_CHUNK) for n in (edge - 1, edge, edge + 1)))
assert max(SEAM_NS) <= 100000


def compensated_only(lm):
    """The ListMode over lm's records with its compensation and nothing else."""
    from chronoclust_amd import _lib
    t = lm.transform
    only = _lib.ListTransform(t.comp_cols, t.comp) if t is not None and t.m else None
    return _lib.ListMode(lm.buffer, lm.n, lm.src_cols, lm.dtype, columns=lm.columns, masks=lm.masks, transform=only)


def referee(sources, q, want=None):
    """(count, lo, hi, frac, r), each [d]: count -1 and zeros for a dimension that is not wanted; r = np.quantile(neg, q), NaN
    where there is no negative value."""
    vals = [np.asarray(compensated_only(s), dtype=np.float64) for s in sources]
    d = vals[0].shape[1]
    count = np.full(d, -1, np.int64)
    lo, hi, frac, r = np.zeros(d), np.zeros(d), np.zeros(d), np.full(d, np.nan)
    for c in range(d):
        if want is not None and not want[c]:
            continue
        v = np.concatenate([x[:, c] for x in vals])
        neg = np.sort(v[v < 0])
        cnt = count[c] = neg.size
        if cnt == 0:
            continue
        h = (cnt - 1) * float(q)
        j = int(np.floor(h))
        lo[c], hi[c], frac[c] = neg[j], neg[min(j + 1, cnt - 1)], h - j
        with np.errstate(all="ignore"):
            r[c] = np.quantile(neg, q)
    return count, lo, hi, frac, r


def width(cnt, r, T, M):
    """W = 0 without a negative value, else (M - log10(T / |r|)) / 2 clamped to [0, M / 2]."""
    if cnt == 0:
        return 0.0
    W = (M - np.log10(T / abs(r))) / 2
    return float(min(max(W, 0.0), M / 2))


def same(got, exp, what):
    """count equal, lo / hi / frac bit for bit; and numpy's interpolation of (lo, hi) at frac has the bits of np.quantile."""
    count, lo, hi, frac, r = exp
    assert np.array_equal(got[0], count), "%s: count %r / %r" % (what, got[0].tolist(), count.tolist())
    U.same_bits(got[1], lo, what + ": lo")
    U.same_bits(got[2], hi, what + ": hi")
    U.same_bits(got[3], frac, what + ": frac")
    for c in np.flatnonzero((count > 0) & np.isfinite(r)):  # (-Inf at the quantile: numpy's own answer is a NaN of no fixed sign)
        with np.errstate(all="ignore"):
            mine = np.quantile(np.array([got[1][c], got[2][c]]), got[3][c])
        U.same_bits(np.array([mine]), np.array([r[c]]), "%s: the interpolation, dimension %d" % (what, c))


def case(n, d, m, dtype, order, seed):
    """A ListMode of n events with test_fcs_transform's layout (compensated columns that are not selected, selected ones that
    are not compensated, a repeated column, masks on the integers), a spillover of its own and cofactors that must be
    ignored.  Floating records straddle zero; integer records turn negative through the compensation alone."""
    import test_fcs_transform as X
    from chronoclust_amd import _lib
    src_cols, cols, comp_cols = X.layout(d, m, seed)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        rec = np.random.default_rng(seed + 1).normal(40.0, 300.0, (n, src_cols)).astype(dtype)
    else:
        rec = U.records(dtype, n, src_cols, seed + 1)
    masks = None
    if dtype.kind == "u":
        masks = [(0x7FFF, 0x3FF, 0xFFFFFFFF, 0xFFF)[c % 4] for c in range(d)]
        if d > 1:
            masks[-1] = masks[0]
    inv = U.spillover(m, seed + 2)[1] if m else None
    tr = _lib.ListTransform(comp_cols if m else None, inv, np.where(np.arange(d) % 2 == 0, 150.0, 0.0))
    return U.list_mode(rec, order, cols, masks, tr)


# ---- designed keys: native float64 records, no compensation; one column per set, padded with +1.0 (which is not counted) -------

BASE = 0xBF38123456789ABC  # a negative double whose eight bytes all differ; its second byte keeps the exponent off all-ones


def from_bits(words):
    return np.array(words, dtype=np.uint64).view(np.float64)


def digit_set(p, count=48):
    """Negative values whose bit patterns differ in byte p alone (0: the most significant): only pass p of the selection finds
    more than one digit among them."""
    shift = 56 - 8 * p
    lo = 0x80 if p == 0 else 0  # (the sign stays set)
    digits = np.random.default_rng(p).permutation(np.arange(lo, 256))[:count]
    return from_bits([(BASE & ~(0xFF << shift)) | (int(g) << shift) for g in digits])


def designed():
    """{name: values}: the sets of the issue; designed_properties checks what each claims."""
    tie = np.concatenate([np.full(26, -5.0), np.full(30, -4.0), np.full(45, -3.0)])  # 101 values: h = 100 q
    sets = {
        "lowest mantissa byte": -1.0 - np.arange(200) * 2.0 ** -52,
        "exponent only": -(2.0 ** np.arange(-500, 501, 10)),
        "all equal": np.full(150, -3.25),
        "heavy ties": tie,
        "cnt 0": np.array([1.0, 2.0]),
        "cnt 1": np.array([-7.5, 3.0]),
        "cnt 2": np.array([-7.5, 3.0, -0.125]),
        "negative subnormals": -np.arange(1, 120) * 5e-324,
        "zeros": np.array([-0.0, 0.0, -0.0, -2.0, -1.0, 0.0, 5.0]),
        "NaN": np.concatenate([from_bits([0x7FF8000000000000, 0xFFF8000000000000, 0xFFF0000000000001, 0x7FF0000000000001]),
                               -np.arange(1.0, 40.0)]),
        "-Inf": np.concatenate([[-np.inf], -np.arange(1.0, 30.0), [np.inf]]),
    }
    for p in range(8):
        sets["digit %d" % p] = digit_set(p)
    return sets


def designed_records(seed=0):
    """(native float64 records [n, sets], names): every set a column in an order of its own, padded with +1.0."""
    sets = designed()
    names = sorted(sets)
    n = max(len(v) for v in sets.values()) + 3
    rec = np.ones((n, len(names)))
    rng = np.random.default_rng(seed)
    for c, name in enumerate(names):
        rows = rng.permutation(n)[:len(sets[name])]
        rec[rows, c] = sets[name]
    return rec, names


def keys(v):
    """The selection's keys of negative values: the complement of the bit pattern."""
    return ~np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def digits_that_differ(v):
    """The bytes (0: most significant) in which the keys of the negative values of v take more than one value."""
    k = keys(v[v < 0])
    return [p for p in range(8) if len(set(((k >> np.uint64(56 - 8 * p)) & np.uint64(255)).tolist())) > 1]
