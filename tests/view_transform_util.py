"""What the tests of the `_view_xl` route share: arrays of the nine view element types in every layout a view takes, the
transform over a view's columns, and the referee - every value of the nine types is exact in double, so the widened values laid
out as native-order float64 event records and sent through the `_list_xl` route with the same transform are what the view route
must hold, bit for bit."""
import numpy as np

import transform_util as U

TYPES = (np.float64, np.float32, np.float16, np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32)
ROWS_LAYOUTS = ("c", "pitch", "wasteful")           # dense, a range of columns of a C-order array, a pitch beyond 8 d (host packing)
COLS_LAYOUTS = ("f", "frange", "transpose")         # dense Fortran order, a range of rows of a Fortran array (cs > n), a transpose
LAYOUTS = ROWS_LAYOUTS + COLS_LAYOUTS
LOGICLE = (262144.0, 0.5, 4.5, 0.0)


def values(dtype, n, d, seed):
    """Native [n, d] of the type: the whole range of the narrow integers, up to 2^18 in magnitude and some negative for the
    rest (compensated events are), finite for float16."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype.kind == "f":
        top = 2.0 ** 15 if dtype.itemsize == 2 else 2.0 ** 18
        return (rng.uniform(-0.3, 1.0, (n, d)) ** 3 * top).astype(dtype)
    info = np.iinfo(dtype)
    lo, hi = (info.min, info.max) if dtype.itemsize < 4 else (max(info.min, -(2 ** 18)), 2 ** 18)
    return rng.integers(lo, hi, (n, d), dtype=dtype, endpoint=True)


def laid_out(a, layout):
    """The same values in another layout: an array that compares equal to `a` and whose strides are the layout's."""
    n, d = a.shape
    if layout == "c":
        out = np.ascontiguousarray(a)
    elif layout == "pitch":
        big = np.zeros((n, d + 5), a.dtype)
        out = big[:, 3:3 + d]
    elif layout == "wasteful":
        big = np.zeros((n, 8 * d + 3), a.dtype)
        out = big[:, 2:2 + d]
    elif layout == "f":
        out = np.asfortranarray(a)
    elif layout == "frange":
        big = np.zeros((n + 7, d), a.dtype, order="F")
        out = big[4:4 + n]
    elif layout == "transpose":
        out = np.zeros((d, n), a.dtype).T
    else:
        raise ValueError(layout)
    out[...] = a
    assert np.ascontiguousarray(out).tobytes() == np.ascontiguousarray(a).tobytes()  # (a NaN too)
    return out


def comp_cols(d, m, seed):
    """min(m, d) distinct columns of 0 .. d - 1 in an order that is not ascending; where d crosses a 64-dimension block, columns
    on both sides of every boundary are among them (d = 130, m >= 3: 3, 64 and 129)."""
    m = min(m, d)
    rng = np.random.default_rng(seed)
    forced = [c for c in ((3, 64, 129) if d == 130 else (64, 63) if d > 64 else ()) if c < d][:m]
    rest = [int(c) for c in rng.permutation(d) if int(c) not in forced]
    cols = forced + rest[:m - len(forced)]
    return np.array([cols[i] for i in rng.permutation(len(cols))], np.int64)


def transform(d, m, seed, cofactor=None, logicle=None):
    """The ListTransform over a view's d columns: min(m, d) compensated columns with the inverse of a spillover matrix."""
    from chronoclust_amd import _lib
    cc = comp_cols(d, m, seed)
    inv = U.spillover(len(cc), seed + 2)[1] if len(cc) else None
    return _lib.ListTransform(cc if len(cc) else None, inv, cofactor, logicle), cc, inv


def cofactors(kind, d):
    """none / a scalar / one per dimension with zeros on every third"""
    if kind == "none":
        return None
    if kind == "scalar":
        return 5.0
    return np.where(np.arange(d) % 3 == 1, 0.0, 150.0)


def logicle_rows(kind, d, cofactor):
    """none / every dimension without a cofactor / some of them / a [d, 4] array of rows that are all off"""
    if kind == "none":
        return None
    cof = np.zeros(d) if cofactor is None else np.broadcast_to(np.asarray(cofactor, np.float64), (d,))
    rows = np.zeros((d, 4))
    if kind != "off":
        free = np.flatnonzero(~(cof > 0))
        rows[free[::(1 if kind == "all" else 2)]] = LOGICLE
    return rows


def widened(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def referee_source(a, tr):
    """The widened values as native-order float64 event records, one byte past an aligned address, with the same transform: the
    ListMode the `_list_xl` route - the parent's kernels - takes."""
    return U.list_mode(widened(a), U.LITTLE if np.little_endian else U.BIG, None, None, tr)


def resident(h, d):
    return h.points_download(d), h.points_download_xt(d)
