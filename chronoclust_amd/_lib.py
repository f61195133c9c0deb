"""Thin ctypes binding of include/chronoclust_hip.h.  Fails loudly when the HIP library or a GPU is missing:
there is no CPU fallback anywhere in this package."""
import ctypes as C
import os

import numpy as np

from . import build as _build

PCORE, OUTLIER = 0, 1
MAX_DIM = 1024

_ERRORS = {-1: "no HIP device / HIP runtime error", -2: "bad argument", -3: "non-finite input", -4: "out of memory",
           -5: "internal error", -6: "exchange between ranks failed"}


class ChronoclustHipError(RuntimeError):
    pass


class CcParams(C.Structure):
    _fields_ = [("eps_sq", C.c_double), ("delta_sq", C.c_double), ("k", C.c_double), ("beta", C.c_double),
                ("mu", C.c_double), ("omicron", C.c_double), ("ups_eps", C.c_double), ("ups_eps_sq", C.c_double),
                ("delta", C.c_double), ("pi", C.c_int32), ("pad", C.c_int32)]


class CcTuning(C.Structure):
    _fields_ = [("window", C.c_int32), ("rounds", C.c_int32), ("segments", C.c_int32),
                ("windows_per_sync", C.c_int32), ("time_kernels", C.c_int32), ("dirty_segments", C.c_int32),
                ("early_window", C.c_int32), ("lookahead", C.c_int32), ("sequential", C.c_int32)]


class CcStats(C.Structure):
    _fields_ = [("points", C.c_int64), ("windows", C.c_int64), ("rounds", C.c_int64), ("truncated", C.c_int64),
                ("scan_launches", C.c_int64), ("scan_ms", C.c_double), ("scan_pair_dims", C.c_double),
                ("run_ms", C.c_double), ("rows", C.c_int64), ("table_rows_scanned", C.c_int64),
                ("lookahead_windows", C.c_int64), ("sharded_windows", C.c_int64), ("comm_launches", C.c_int64),
                ("comm_ms", C.c_double), ("seq_points", C.c_int64), ("scan_u_launches", C.c_int64),
                ("scan_p_launches", C.c_int64), ("pruned_scan_rows", C.c_int64), ("pruned_scan_full_rows", C.c_int64),
                ("window", C.c_int64), ("long_chains", C.c_int64), ("long_chain_launches", C.c_int64),
                ("tiles", C.c_int64), ("dirty_tiles", C.c_int64),
                ("scan_launches_pruned", C.c_int64), ("scan_ms_pruned", C.c_double), ("scan_pair_dims_pruned", C.c_double),
                ("scan_g_launches", C.c_int64), ("missed_points", C.c_int64), ("probe_launches", C.c_int64),
                ("seq_r_points", C.c_int64), ("heavy_launches", C.c_int64),
                ("scan_lean_launches", C.c_int64), ("long_prepared", C.c_int64), ("long_replayed", C.c_int64),
                ("seq_g_points", C.c_int64), ("link_launches", C.c_int64),
                ("scan_p2_launches", C.c_int64),
                ("calib_allgather_us", C.c_double), ("calib_scan_ns_per_row_dim", C.c_double),
                ("split_threshold_row_dims", C.c_int64), ("split_threshold_row_dims_pruned", C.c_int64),
                ("missed_plain_launches", C.c_int64), ("seed16_launches", C.c_int64),
                ("pad_rows_launches", C.c_int64), ("assign_points", C.c_int64), ("assign_launches", C.c_int64)]


POLICY_MAX_ROUNDS = 8


class CcPolicyConfig(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("window", "rounds_max", "windows_per_sync", "early_window", "lookahead",
                                         "allow_nodirty", "prune_mode", "prune_applicable", "can_shard", "d", "resume",
                                         "allow_sparse", "allow_guess", "allow_probe")] + \
               [("shard_min_row_dims", C.c_int64), ("n_end", C.c_int64), ("shard_min_row_dims_pruned", C.c_int64),
                ("lookahead_pruned", C.c_int32), ("force_prune_rows", C.c_int32)]


class CcPolicyCarry(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("adapt_win", "clean_batches", "since_shrink", "pad")]


class CcPolicyObs(C.Structure):
    _fields_ = [("cursor", C.c_int64), ("m_rows", C.c_int32), ("stall_b", C.c_int32)] + \
               [(k, C.c_int64) for k in ("stat_windows", "stat_truncated", "stat_trunc_unknown", "stat_tiles",
                                         "stat_dirty_tiles", "stat_unsafe", "stat_missed")] + \
               [("round_hist", C.c_int64 * (POLICY_MAX_ROUNDS + 2)), ("prune_rows", C.c_uint64), ("prune_full", C.c_uint64),
                ("after_sequential", C.c_int32), ("tg_ok", C.c_int32)]


class CcPolicyDecision(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("win_cfg", "want", "rounds", "batch_windows", "lookahead", "nodirty", "prune",
                                         "shard", "restart", "bad", "stalled", "sparse", "probe", "pad")] + \
               [(k, C.c_int64) for k in ("wins", "pts", "trunc", "unk", "tiles", "dtiles", "grew", "prune_rows", "prune_full")]


class CcSeqEvent(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("chunk_event", "bad", "possible", "more", "seq_r_applies", "use_g", "allow_seq_g", "wide")] + \
               [("got", C.c_int64), ("chunk", C.c_int64), ("rate", C.c_double), ("rate_guess", C.c_double)]


class CcBatchInputs(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("window", "win_cfg", "S_cfg", "n_cus", "prune_now", "prune_wgs_per_cu", "plain_wgs_per_cu",
                                         "decide_threads", "chain_threads", "commit_threads", "allow_claims", "allow_long",
                                         "allow_heavy", "allow_prep", "m_rows", "n_heavy", "long_seen", "long_few")] + \
               [("long_avg", C.c_int64), ("batch_windows", C.c_int32), ("pad", C.c_int32), ("points_left", C.c_int64)]


LONG_NONE, LONG_ROWS_SPLIT, LONG_ROWS_SMALL, LONG_LIST_SPLIT, LONG_LIST_SMALL = range(5)


class CcBatchGeometry(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("gw", "S", "sparse_cap", "dblocks", "cblocks", "rblocks", "scan_rows", "long_rows",
                                         "long_listed", "heavy_on", "long_cap", "windows_now", "prep", "prep_form", "long_form",
                                         "pad")]


class CcPointsView(C.Structure):
    """cc_points_view: points where they lie; strides in elements."""
    _fields_ = [("data", C.c_void_p), ("n", C.c_int64), ("d", C.c_int32), ("dtype", C.c_int32),
                ("row_stride", C.c_int64), ("col_stride", C.c_int64)]


# CC_DT_*: the element types a view may have, by numpy dtype (native byte order)
DT_F64, DT_F32, DT_F16, DT_I8, DT_U8, DT_I16, DT_U16, DT_I32, DT_U32 = range(9)
VIEW_DTYPES = {np.dtype(t): code for t, code in (
    (np.float64, DT_F64), (np.float32, DT_F32), (np.float16, DT_F16), (np.int8, DT_I8), (np.uint8, DT_U8),
    (np.int16, DT_I16), (np.uint16, DT_U16), (np.int32, DT_I32), (np.uint32, DT_U32))}


class CcListMode(C.Structure):
    """cc_list_mode: list-mode event records as the bytes an FCS DATA segment holds."""
    _fields_ = [("data", C.c_void_p), ("n", C.c_int64), ("src_cols", C.c_int32), ("dtype", C.c_int32),
                ("flags", C.c_int32), ("d", C.c_int32), ("cols", C.POINTER(C.c_int32)), ("masks", C.POINTER(C.c_uint32))]


class CcListTransform(C.Structure):
    """cc_list_transform: compensation and arcsinh of list-mode event records on the device."""
    _fields_ = [("m", C.c_int32), ("reserved", C.c_int32), ("comp_cols", C.POINTER(C.c_int32)),
                ("comp", C.POINTER(C.c_double)), ("cofactor", C.POINTER(C.c_double))]


class CcListLogicle(C.Structure):
    """cc_list_logicle: the logicle scale of list-mode event records on the device, one row T, W, M, A per selected dimension."""
    _fields_ = [("d", C.c_int32), ("reserved", C.c_int32), ("twma", C.POINTER(C.c_double))]


LM_SWAPPED = 1
MAX_SRC_COLS = 4096
MAX_COMP = 64
# the element types list-mode data has, by numpy dtype in native byte order
LIST_DTYPES = {np.dtype(t): code for t, code in (
    (np.float32, DT_F32), (np.float64, DT_F64), (np.uint8, DT_U8), (np.uint16, DT_U16), (np.uint32, DT_U32))}


class ListTransform(object):
    """What list-mode events take before they are clustered (cc_list_transform), applied on the device as they land:
    comp_cols: m distinct source columns (indices into the record) and comp: [m, m], the INVERSE of their spillover matrix - a
    selected dimension whose source column is comp_cols[i] becomes sum_j x[comp_cols[j]] * comp[j, i], summed left to right in
    double, nothing fused; compensated columns need not be selected.  cofactor: a number for every selected dimension or one
    per selected dimension; > 0: arcsinh(v / cofactor), 0: the value passes through.  logicle: one (T, W, M, A) for every
    selected dimension, or a [d, 4] array whose rows with T == 0 leave their dimension off the scale - the logicle (biexponential)
    display scale of Moore and Parks 2012 on the unit scale (T maps to 1, 0 to x1 = (A + W) / (M + A)), after the compensation,
    in the place of a cofactor: a dimension takes one or the other (ListMode refuses one that carries both).  Attached through
    ListMode(..., transform=...).  Only the shapes are checked here and the values are the library's to refuse (ValueError) -
    but for the logicle rows, which the library checks at once (logicle_coefficients: no GPU needed)."""

    def __init__(self, comp_cols=None, comp=None, cofactor=None, logicle=None):
        if (comp_cols is None) != (comp is None):
            raise ValueError("ListTransform: comp_cols and comp go together")
        self.comp_cols = np.zeros(0, np.int32) if comp_cols is None else np.ascontiguousarray(comp_cols, dtype=np.int32)
        m = self.m = int(self.comp_cols.size)
        if self.comp_cols.ndim != 1:
            raise ValueError("ListTransform: comp_cols must be a list of indices")
        self.comp = np.zeros((0, 0)) if comp is None else np.ascontiguousarray(comp, dtype=np.float64)
        if self.comp.shape != (m, m):
            raise ValueError("ListTransform: comp must be [%d, %d], one row and one column per compensated column" % (m, m))
        if cofactor is not None:
            cofactor = np.asarray(cofactor, dtype=np.float64)
            cofactor = cofactor if cofactor.ndim == 0 else np.ascontiguousarray(cofactor)
            if cofactor.ndim > 1:
                raise ValueError("ListTransform: cofactor is a number or one number per selected dimension")
        self.cofactor = cofactor
        if logicle is not None:
            logicle = np.ascontiguousarray(logicle, dtype=np.float64)
            if logicle.shape != (4,) and (logicle.ndim != 2 or logicle.shape[1] != 4):
                raise ValueError("ListTransform: logicle is one (T, W, M, A) or a [d, 4] array of them")
            for row in logicle.reshape(-1, 4):
                logicle_coefficients(row)  # (the library's own refusals, before any handle exists: ValueError)
        self.logicle = logicle

    def logicles(self, d):
        """The d rows T, W, M, A ([d, 4]; one row given is every dimension's), or None."""
        if self.logicle is None:
            return None
        if self.logicle.ndim == 1:
            return np.ascontiguousarray(np.tile(self.logicle, (d, 1)))
        if self.logicle.shape != (d, 4):
            raise ValueError("ListTransform: %d logicle rows for %d selected dimensions" % (self.logicle.shape[0], d))
        return self.logicle

    def cofactors(self, d):
        """The d cofactors (a number is every dimension's), or None."""
        if self.cofactor is None:
            return None
        if self.cofactor.ndim == 0:
            return np.full(d, float(self.cofactor))
        if self.cofactor.shape != (d,):
            raise ValueError("ListTransform: %d cofactors for %d selected dimensions" % (self.cofactor.size, d))
        return self.cofactor


class ListMode(object):
    """List-mode event records where they lie (cc_list_mode): `buffer` holds n records of src_cols elements of `dtype` - a
    numpy dtype WITH its byte order, float32 / float64 / uint8 / uint16 / uint32 -, of which `columns` (indices into the
    record, any order, repeats allowed; None: all of them) are the dimensions, the integer ones ANDed with `masks` (one per
    selected column; None: none).  The buffer may start at any address and is kept alive by this object; it is never copied
    or packed on the host: the `_list` entry points move whole records and the device swaps, gathers, masks and widens.
    shape == (n, d), ndim == 2; np.asarray(list_mode) is the host decode - float32 for float32 sources, else float64 -, the
    referee of the device route and the fallback of every host-side consumer.
    transform: a ListTransform - the records then go through the `_list_xf` entry points and are compensated and
    arcsinh-transformed on the device.  np.asarray(list_mode) applies the transform on the host (always float64): the same
    left-to-right sum in numpy, which IS the device's compensation bit for bit, and np.arcsinh, which agrees with the device's
    asinh only to a few units in the last place (tests/test_fcs_transform.py keeps the measured bound), not bit for bit - so
    what the device holds is read back from it (Handle.points_download) wherever the very values matter.
    With a logicle row that is on (T > 0) the records go through the `_list_xl` entry points and the scale is solved on the
    device; np.asarray(list_mode) solves it in numpy from the library's own coefficients (logicle_coefficients), the same
    iteration with numpy's expm1 and log: device and host each lie within a few units of np.spacing(max(|y|, 0.5)) of the true
    root and agree to the sum of their bounds, not bit for bit."""

    ndim = 2

    def __init__(self, buffer, n, src_cols, dtype, columns=None, masks=None, transform=None):
        dtype = np.dtype(dtype)
        if dtype.newbyteorder("=") not in LIST_DTYPES:
            raise ValueError("ListMode: dtype %s is none of float32, float64, uint8, uint16, uint32" % dtype)
        n, src_cols = int(n), int(src_cols)
        if n < 0 or src_cols < 1:
            raise ValueError("ListMode: n must be non-negative and src_cols positive")
        self._bytes = np.frombuffer(buffer, dtype=np.uint8)  # (keeps the buffer alive; any address)
        if self._bytes.size < n * src_cols * dtype.itemsize:
            raise ValueError("ListMode: the buffer holds %d bytes, %d records of %d x %s need %d"
                             % (self._bytes.size, n, src_cols, dtype, n * src_cols * dtype.itemsize))
        self.buffer = buffer
        self.n, self.src_cols, self.dtype = n, src_cols, dtype
        self.swapped = not dtype.isnative
        self.columns = np.arange(src_cols, dtype=np.int32) if columns is None else np.ascontiguousarray(columns, dtype=np.int32)
        if self.columns.ndim != 1 or self.columns.size < 1:
            raise ValueError("ListMode: columns must be a non-empty list of indices")
        if self.columns.min() < 0 or self.columns.max() >= src_cols:
            raise ValueError("ListMode: a column is outside 0..%d" % (src_cols - 1))
        self.masks = None
        if masks is not None:
            if dtype.kind != "u":
                raise ValueError("ListMode: masks are for the integer dtypes only")
            self.masks = np.ascontiguousarray(masks, dtype=np.uint32)
            if self.masks.shape != self.columns.shape:
                raise ValueError("ListMode: one mask per selected column")
        self.shape = (n, int(self.columns.size))
        self.transform = transform
        self._cofactors, self._logicle = _transform_rows(transform, self.shape[1], "ListMode")

    def __len__(self):
        return self.n

    def descriptor(self):
        """The cc_list_mode of these records (it points into this object: keep it alive while the descriptor is used)."""
        return CcListMode(self._bytes.ctypes.data if self._bytes.size else None, self.n, self.src_cols,
                          LIST_DTYPES[self.dtype.newbyteorder("=")], LM_SWAPPED if self.swapped else 0, self.shape[1],
                          self.columns.ctypes.data_as(C.POINTER(C.c_int32)),
                          None if self.masks is None else self.masks.ctypes.data_as(C.POINTER(C.c_uint32)))

    def transform_descriptor(self):
        """The cc_list_transform of these records, or None without one (it points into this object, as descriptor())."""
        t = self.transform
        if t is None:
            return None
        return CcListTransform(t.m, 0, t.comp_cols.ctypes.data_as(C.POINTER(C.c_int32)) if t.m else None,
                               t.comp.ctypes.data_as(C.POINTER(C.c_double)) if t.m else None,
                               None if self._cofactors is None else self._cofactors.ctypes.data_as(C.POINTER(C.c_double)))

    def logicle_descriptor(self):
        """The cc_list_logicle of these records, or None where no row is on (it points into this object, as descriptor())."""
        if self._logicle is None:
            return None
        return CcListLogicle(self.shape[1], 0, self._logicle.ctypes.data_as(C.POINTER(C.c_double)))

    def __array__(self, dtype=None, copy=None):
        rec = np.frombuffer(self._bytes, dtype=self.dtype, count=self.n * self.src_cols).reshape(self.n, self.src_cols)
        native = self.dtype.newbyteorder("=")
        out = rec[:, self.columns]
        if self.masks is not None:
            out = out.astype(native) & self.masks.astype(native)
        if self.transform is not None:
            out = self._host_transform(rec, out.astype(np.float64))
        else:
            out = out.astype(np.float32 if self.dtype.itemsize == 4 and self.dtype.kind == "f" else np.float64)
        return out if dtype is None else out.astype(dtype, copy=False)

    def _host_transform(self, rec, out):
        """The transform on the host, as the device applies it: a compensated column decoded under the mask of the first
        selected dimension that names it, the sum left to right with every product and sum rounded, then arcsinh."""
        t = self.transform
        native = self.dtype.newbyteorder("=")
        cols = self.columns.tolist()
        xs = []
        for c in t.comp_cols.tolist():
            x = rec[:, c].astype(native)
            if self.masks is not None and c in cols:
                x = x & self.masks[cols.index(c)].astype(native)
            xs.append(x.astype(np.float64))
        hits = [np.flatnonzero(t.comp_cols == c) for c in cols]
        return _host_transform(out, xs, [int(h[0]) if h.size else -1 for h in hits], t, self._cofactors, self._logicle)


def _transform_rows(transform, d, who):
    """(cofactors [d] or None, logicle rows [d, 4] or None: every row off is none) of a ListTransform over d dimensions, with
    the refusal of a dimension that carries a cofactor and a logicle scale - what ListMode and TransformedPoints (`who`) keep."""
    if transform is None:
        return None, None
    if not isinstance(transform, ListTransform):
        raise ValueError("%s: transform must be a ListTransform" % who)
    cofactors = transform.cofactors(d)
    logicle = transform.logicles(d)
    if logicle is not None and not (logicle[:, 0] != 0).any():
        logicle = None  # (every row off: the sibling without logicle rows)
    if logicle is not None and cofactors is not None:
        both = np.flatnonzero((logicle[:, 0] != 0) & (cofactors > 0))
        if both.size:
            raise ValueError("%s: dimension %d has a cofactor and a logicle scale" % (who, both[0]))
    return cofactors, logicle


def _host_transform(out, xs, hits, t, cofactors, logicle):
    """The transform on the host over out [n, d] float64, the dimensions' own values, in place: xs the m compensated columns
    as float64, hits[k] the index of dimension k among them or -1; the sum left to right with every product and sum rounded,
    then arcsinh, then the logicle scale - ListMode's and TransformedPoints' one implementation."""
    for k, i in enumerate(hits):
        if i >= 0:
            v = xs[0] * t.comp[0, i]
            for j in range(1, t.m):
                v = v + xs[j] * t.comp[j, i]
            out[:, k] = v
    if cofactors is not None:
        with np.errstate(all="ignore"):
            for k, cf in enumerate(cofactors.tolist()):
                if cf > 0:
                    out[:, k] = np.arcsinh(out[:, k] / cf)
    if logicle is not None:
        for k, row in enumerate(logicle):
            if row[0] != 0:
                out[:, k] = logicle_host(out[:, k], row)
    return out


class TransformedPoints(object):
    """An [n, d] array of points with a ListTransform the device applies while it takes them in (the `_view_xl` entry points):
    what ListMode(..., transform=...) is for `.fcs` events, for the arrays a parsed CSV, a `.npy` file or a caller hands over.
    transform.comp_cols index the ARRAY's columns 0 .. d - 1 - every compensated column is a dimension -, cofactor and
    logicle hold one entry / one row per column (or one for all).  The contract is ListTransform's: the left-to-right sum in
    double, arcsinh(v / cofactor) or the logicle scale, a dimension takes one or the other.
    An array points_view accepts - the nine element types, rows or columns form, C-contiguous float32 / float64 included - is
    read where it lies; anything else is copied once, here, to C-contiguous float64 and that copy is read.
    shape == (n, d), ndim == 2; np.asarray(points) applies the transform on the host (always float64), by the implementation
    ListMode has: the device's compensation bit for bit, its asinh and logicle solve to a few units in the last place - where
    the very values matter, read them back (Handle.points_download)."""

    ndim = 2

    def __init__(self, array, transform):
        array = np.asarray(array)
        if array.ndim != 2:
            raise ValueError("TransformedPoints: the points must be a 2-d array")
        self.array = array
        self.shape = tuple(int(v) for v in array.shape)
        self.transform = transform
        self._cofactors, self._logicle = _transform_rows(transform, self.shape[1], "TransformedPoints")
        # what the library reads: the array where it lies, or a C-contiguous float64 copy of it
        self.points = array if points_view(array) is not None or self.shape[0] == 0 else _f64(array)

    def __len__(self):
        return self.shape[0]

    def descriptor(self):
        """The cc_points_view of these points (it points into this object: keep it alive while the descriptor is used)."""
        view = points_view(self.points)
        return view if view is not None else CcPointsView(None, self.shape[0], self.shape[1], DT_F64, max(self.shape[1], 1), 1)

    transform_descriptor = ListMode.transform_descriptor
    logicle_descriptor = ListMode.logicle_descriptor

    def __array__(self, dtype=None, copy=None):
        t = self.transform
        out = np.array(self.array, dtype=np.float64, order="C")
        if t is not None:
            cols = t.comp_cols.tolist()
            if any(c < 0 or c >= self.shape[1] for c in cols):
                raise ValueError("TransformedPoints: a compensated column is outside 0..%d" % (self.shape[1] - 1))
            xs = [np.asarray(self.array[:, c], dtype=np.float64) for c in cols]
            hits = [cols.index(k) if k in cols else -1 for k in range(self.shape[1])]
            out = _host_transform(out, xs, hits, t, self._cofactors, self._logicle)
        return out if dtype is None else out.astype(dtype, copy=False)


LOGICLE_STEPS = 4  # (CC_LOGICLE_STEPS of csrc/cc_ingest_list_xf.h)


def logicle_coefficients(twma):
    """cc_logicle_coefficients: (x1, b, d, pa, pc) of one logicle scale (T, W, M, A) as the kernels receive them, derived by the
    library (no GPU needed); all zeros for T == 0.  ValueError for parameters outside the contract: T >= 0, M > 0, 0 <= W,
    2 W <= M, -W <= A <= M - 2 W, all finite."""
    twma = np.ascontiguousarray(twma, dtype=np.float64)
    if twma.shape != (4,):
        raise ValueError("logicle_coefficients: one (T, W, M, A)")
    out = np.zeros(8)
    rc = load().cc_logicle_coefficients(twma.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != 0:
        raise ValueError("logicle (T, W, M, A) = %r is outside T >= 0, M > 0, 0 <= W, 2 W <= M, -W <= A <= M - 2 W, all finite"
                         % (tuple(twma.tolist()),))
    return tuple(out[:5].tolist())


def logicle_host(v, twma):
    """logicle(v) of a float64 array on the host, vectorised: cc_logicle_value of csrc/cc_ingest_list_xf.h restated in numpy -
    the same start, the same LOGICLE_STEPS Halley steps in the expm1 form, the same operations in the same order - from the
    library's own coefficients, in pieces of 64 Ki values so that the temporaries stay in cache.  A NaN or Inf gives a
    non-finite result."""
    x1, b, d, pa, pc = logicle_coefficients(twma)
    v = np.asarray(v, dtype=np.float64)
    flat = np.ascontiguousarray(v).reshape(-1)
    out = np.empty_like(flat)
    kc = pc / pa
    kd = kc * d
    with np.errstate(all="ignore"):
        for at in range(0, flat.size, 1 << 16):
            w = flat[at:at + (1 << 16)]
            y = np.abs(w)
            r = y / pa
            u = np.minimum(r / (b + kd), np.log(r + 1.0) / b)
            for _ in range(LOGICLE_STEPS):
                e1 = np.expm1(b * u)
                e2 = np.expm1(-(d * u))
                f = (e1 - kc * e2) - r
                p1 = b * (e1 + 1.0)
                p2 = kd * (e2 + 1.0)
                f1 = p1 + p2
                f2 = b * p1 - d * p2
                q = f / f1
                u = u - q / (1.0 - 0.5 * (q * (f2 / f1)))
            far = ~(r <= 2.0 ** 900)
            if far.any():
                u[far] = (np.log(y[far]) - np.log(pa)) / b
            out[at:at + (1 << 16)] = np.where(w < 0.0, x1 - u, x1 + u)
    return out.reshape(v.shape)


def _negq_sources(sources, want):
    """(sources as a list, d, want as a uint8 mask [d] or None) of what negative_quantiles and its host sibling are given."""
    sources = list(sources)
    if not sources or not all(isinstance(s, ListMode) for s in sources):
        raise ValueError("negative_quantiles: sources must be a non-empty list of ListMode")
    d = sources[0].shape[1]
    if any(s.shape[1] != d for s in sources):
        raise ValueError("negative_quantiles: every source must select %d dimensions" % d)
    if want is not None:
        want = np.ascontiguousarray(np.asarray(want).astype(bool), dtype=np.uint8)
        if want.shape != (d,):
            raise ValueError("negative_quantiles: want must hold one entry per selected dimension")
    return sources, d, want


def compensation_only(source):
    """The ListMode over the same records with the compensation of its transform and nothing else: no cofactors, no logicle
    rows - what the negative quantiles are taken of."""
    t = source.transform
    if t is None or (source._cofactors is None and source._logicle is None):
        return source
    only = ListTransform(t.comp_cols, t.comp) if t.m else None
    return ListMode(source.buffer, source.n, source.src_cols, source.dtype, columns=source.columns, masks=source.masks, transform=only)


def negative_quantiles_host(sources, q=0.05, want=None):
    """Handle.negative_quantiles on the host: (count, lo, hi, frac) from np.asarray of every source with its compensation only
    (the device's sum, bit for bit), pooled - the route where there is no handle."""
    sources, d, want = _negq_sources(sources, want)
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError("negative_quantiles: q must be in [0, 1]")
    vals = [np.asarray(compensation_only(s), dtype=np.float64) for s in sources]
    count = np.full(d, -1, np.int64)
    lo, hi, frac = np.zeros(d), np.zeros(d), np.zeros(d)
    for c in range(d):
        if want is not None and not want[c]:
            continue
        col = np.concatenate([v[:, c] for v in vals])
        neg = np.sort(col[col < 0])
        count[c] = neg.size
        if neg.size:
            h = np.float64(neg.size - 1) * np.float64(q)
            j = int(np.floor(h))
            lo[c], hi[c], frac[c] = neg[j], neg[min(j + 1, neg.size - 1)], h - np.floor(h)
    return count, lo, hi, frac


class CcRelaxedStats(C.Structure):
    _fields_ = [("super_steps", C.c_int64), ("minibatch_points", C.c_int64), ("deferred_points", C.c_int64),
                ("reserved", C.c_int64 * 5)]


_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_i8p = C.POINTER(C.c_int8)
_vp = C.POINTER(CcPointsView)
_lp = C.POINTER(CcListMode)
_xp = C.POINTER(CcListTransform)
_gp = C.POINTER(CcListLogicle)

# name -> (restype, argtypes): every symbol include/chronoclust_hip.h declares
SYMBOLS = {
    "cc_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "cc_destroy": (None, [C.c_void_p]),
    "cc_last_error": (C.c_char_p, [C.c_void_p]),
    "cc_set_tuning": (C.c_int, [C.c_void_p, C.POINTER(CcTuning)]),
    "cc_reset": (C.c_int, [C.c_void_p]),
    "cc_set_params": (C.c_int, [C.c_void_p, C.POINTER(CcParams)]),
    "cc_decay_downgrade": (C.c_int, [C.c_void_p, C.c_double]),
    "cc_points_upload": (C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32]),
    "cc_points_prefetch": (C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, _dp, _dp]),
    "cc_online_run": (C.c_int, [C.c_void_p]),
    "cc_col_minmax": (C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, _dp, _dp]),
    "cc_points_upload_scaled": (C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, _dp, _dp]),
    "cc_points_download": (C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    "cc_labels_download": (C.c_int, [C.c_void_p, _i64p, _i8p]),
    "cc_online": (C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, _i64p, _i8p]),
    "cc_assign": (C.c_int, [C.c_void_p, _dp, C.c_int64, C.c_int32, _i64p, _i8p, _dp]),
    "cc_points_upload_f32": (C.c_int, [C.c_void_p, _fp, C.c_int64, C.c_int32]),
    "cc_points_upload_scaled_f32": (C.c_int, [C.c_void_p, _fp, C.c_int64, C.c_int32, _dp, _dp]),
    "cc_points_prefetch_f32": (C.c_int, [C.c_void_p, _fp, C.c_int64, C.c_int32, _dp, _dp]),
    "cc_col_minmax_f32": (C.c_int, [C.c_void_p, _fp, C.c_int64, C.c_int32, _dp, _dp]),
    "cc_online_f32": (C.c_int, [C.c_void_p, _fp, C.c_int64, C.c_int32, _i64p, _i8p]),
    "cc_assign_f32": (C.c_int, [C.c_void_p, _fp, C.c_int64, C.c_int32, _i64p, _i8p, _dp]),
    "cc_points_download_xt": (C.c_int, [C.c_void_p, _dp]),
    "cc_f32_points": (C.c_int, [C.c_void_p, _i64p]),
    "cc_points_upload_view": (C.c_int, [C.c_void_p, _vp, _dp, _dp]),
    "cc_points_prefetch_view": (C.c_int, [C.c_void_p, _vp, _dp, _dp]),
    "cc_col_minmax_view": (C.c_int, [C.c_void_p, _vp, _dp, _dp]),
    "cc_online_view": (C.c_int, [C.c_void_p, _vp, _i64p, _i8p]),
    "cc_assign_view": (C.c_int, [C.c_void_p, _vp, _i64p, _i8p, _dp]),
    "cc_view_points": (C.c_int, [C.c_void_p, _i64p]),
    "cc_points_upload_view_xl": (C.c_int, [C.c_void_p, _vp, _xp, _gp, _dp, _dp]),
    "cc_points_prefetch_view_xl": (C.c_int, [C.c_void_p, _vp, _xp, _gp, _dp, _dp]),
    "cc_col_minmax_view_xl": (C.c_int, [C.c_void_p, _vp, _xp, _gp, _dp, _dp]),
    "cc_online_view_xl": (C.c_int, [C.c_void_p, _vp, _xp, _gp, _i64p, _i8p]),
    "cc_assign_view_xl": (C.c_int, [C.c_void_p, _vp, _xp, _gp, _i64p, _i8p, _dp]),
    "cc_points_upload_list": (C.c_int, [C.c_void_p, _lp, _dp, _dp]),
    "cc_points_prefetch_list": (C.c_int, [C.c_void_p, _lp, _dp, _dp]),
    "cc_col_minmax_list": (C.c_int, [C.c_void_p, _lp, _dp, _dp]),
    "cc_online_list": (C.c_int, [C.c_void_p, _lp, _i64p, _i8p]),
    "cc_assign_list": (C.c_int, [C.c_void_p, _lp, _i64p, _i8p, _dp]),
    "cc_list_points": (C.c_int, [C.c_void_p, _i64p]),
    "cc_points_upload_list_xf": (C.c_int, [C.c_void_p, _lp, _xp, _dp, _dp]),
    "cc_points_prefetch_list_xf": (C.c_int, [C.c_void_p, _lp, _xp, _dp, _dp]),
    "cc_col_minmax_list_xf": (C.c_int, [C.c_void_p, _lp, _xp, _dp, _dp]),
    "cc_online_list_xf": (C.c_int, [C.c_void_p, _lp, _xp, _i64p, _i8p]),
    "cc_assign_list_xf": (C.c_int, [C.c_void_p, _lp, _xp, _i64p, _i8p, _dp]),
    "cc_points_upload_list_xl": (C.c_int, [C.c_void_p, _lp, _xp, _gp, _dp, _dp]),
    "cc_points_prefetch_list_xl": (C.c_int, [C.c_void_p, _lp, _xp, _gp, _dp, _dp]),
    "cc_col_minmax_list_xl": (C.c_int, [C.c_void_p, _lp, _xp, _gp, _dp, _dp]),
    "cc_online_list_xl": (C.c_int, [C.c_void_p, _lp, _xp, _gp, _i64p, _i8p]),
    "cc_assign_list_xl": (C.c_int, [C.c_void_p, _lp, _xp, _gp, _i64p, _i8p, _dp]),
    "cc_logicle_coefficients": (C.c_int, [_dp, _dp]),
    "cc_negq_begin": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), C.c_int64]),
    "cc_negq_add_list": (C.c_int, [C.c_void_p, _lp, _xp]),
    "cc_negq_select": (C.c_int, [C.c_void_p, C.c_double, _i64p, _dp, _dp, _dp]),
    "cc_negq_end": (C.c_int, [C.c_void_p]),
    "cc_count": (C.c_int, [C.c_void_p, C.c_int]),
    "cc_dim": (C.c_int, [C.c_void_p]),
    "cc_counters": (C.c_int, [C.c_void_p, _i64p, _i64p]),
    "cc_set_counters": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64]),
    "cc_export": (C.c_int, [C.c_void_p, C.c_int, _i64p, _i64p, _dp, _dp, _dp, _dp, _dp]),
    "cc_inject_mc": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, _dp, _dp, _dp, _dp, C.c_double, C.c_int64,
                               C.c_int64]),
    "cc_inject_bulk": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp, _i64p, _i64p]),
    "cc_offline": (C.c_int, [C.c_void_p, _i32p, _i8p, _i32p, _i32p, _i32p]),
    "cc_num_core": (C.c_int, [C.c_void_p]),
    "cc_cluster_size": (C.c_int, [C.c_void_p, C.c_int32]),
    "cc_cluster_export": (C.c_int, [C.c_void_p, C.c_int32, _i64p, _dp, _dp, _dp, _dp, _dp]),
    "cc_clusters_total_members": (C.c_int, [C.c_void_p]),
    "cc_clusters_export": (C.c_int, [C.c_void_p, _i64p, _i32p, _dp, _dp, _dp, _dp, _dp]),
    "cc_assoc_argmin": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int32, _dp, C.c_int32, C.c_int32, _i32p, _dp]),
    "cc_get_stats": (C.c_int, [C.c_void_p, C.POINTER(CcStats)]),
    "cc_sync": (C.c_int, [C.c_void_p]),
    "cc_policy_replay": (C.c_int, [C.POINTER(CcPolicyConfig), C.POINTER(CcPolicyCarry), C.c_int64, C.c_int32,
                                   C.POINTER(CcPolicyObs), C.c_int32, C.POINTER(CcPolicyDecision)]),
    "cc_point_clusters": (C.c_int, [C.c_void_p, _i32p]),
    "cc_format_points_csv": (C.c_int64, [_dp, C.c_int64, C.c_int32, C.c_int64, _i32p, C.c_char_p, _i32p, C.c_int32,
                                         C.c_void_p, C.c_int64]),
    "cc_comm_unique_id": (C.c_int, [C.c_char_p]),
    "cc_comm_init_rccl": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int]),
    "cc_comm_init_local": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "cc_comm_calibrate": (C.c_int, [C.c_void_p]),
    "cc_comm_destroy": (C.c_int, [C.c_void_p]),
    "cc_comm_info": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p]),
    "cc_comm_set_relaxed": (C.c_int, [C.c_void_p, C.c_int32]),
    "cc_get_relaxed_stats": (C.c_int, [C.c_void_p, C.POINTER(CcRelaxedStats)]),
    "cc_policy_seq_rate_guess": (C.c_double, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "cc_seq_handover_replay": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(CcSeqEvent), C.c_int32, _i32p, _i64p]),
    "cc_batch_plan": (C.c_int, [C.POINTER(CcBatchInputs), C.POINTER(CcBatchGeometry)]),
    "cc_scan_width": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _i32p]),
    "cc_shard_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p]),
    "cc_set_shard_thresholds": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32]),
}

COMM_ID_BYTES = 128

_lib = None


def load():
    """Loads libchronoclust_hip.so (built in-tree by chronoclust_amd.build).  Raises if it is missing."""
    global _lib
    if _lib is None:
        path = os.environ.get("CHRONOCLUST_HIP_LIB") or _build.LIB_PATH  # (a build variant, for kernel experiments)
        if not os.path.exists(path):
            raise ChronoclustHipError(
                "HIP library %s not built; run `python -m chronoclust_amd.build` (needs hipcc). "
                "chronoclust_amd has no CPU fallback." % path)
        if _build.is_stale(path) and os.environ.get("CHRONOCLUST_HIP_ALLOW_STALE") != "1":
            # (keyed to the CONTENT of csrc/ and the header, not to file times: the GPU box receives a copy of the tree)
            raise ChronoclustHipError(
                "HIP library %s was not built from the sources beside it (csrc/ or include/chronoclust_hip.h changed since, or "
                "its .sha256 stamp is missing); run `python -m chronoclust_amd.build`." % path)
        lib = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


HOST_ONLY_SYMBOLS = ("cc_policy_replay", "cc_policy_seq_rate_guess", "cc_seq_handover_replay", "cc_batch_plan", "cc_shard_rows",
                     "cc_format_points_csv", "cc_scan_width")


def load_host_only(path):
    """Binds a library that holds only the entry points that are plain host code (csrc/cc_host_abi.inc built by itself: the
    sanitizer builds of tests/host_san/) in the place of the HIP library, so that policy_replay, seq_handover_replay,
    batch_plan, shard_rows and format_points_csv of this module drive it.  Test infrastructure: nothing that needs a handle works afterwards."""
    global _lib
    lib = C.CDLL(path)
    for name in HOST_ONLY_SYMBOLS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = SYMBOLS[name]
    _lib = lib
    return lib


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def is_f32_points(a):
    """True for what the `_f32` entry points take as it is: a C-contiguous 2-d float32 ndarray."""
    return isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.flags["C_CONTIGUOUS"]


def as_points(a):
    """Points as the library takes them without another copy: a C-contiguous 2-d float32 ndarray is returned as it is (the
    very object - the `_f32` entry points read it, the device widens it), everything else - other dtypes, Fortran order,
    strided views, lists - as a C-contiguous float64 array (_f64), as ever."""
    return a if is_f32_points(a) else _f64(a)


def points_view(a):
    """The cc_points_view of a 2-d ndarray the `_view` entry points take as it lies, else None.  Taken: the nine element
    types of VIEW_DTYPES in native byte order, at least one point, and one of two layouts - rows form (columns one element
    apart, rows at least d apart: C order, a range of columns of a C-order array) or columns form (rows one element apart,
    columns at least n apart: Fortran order, a range of rows of a Fortran-order array, a transpose).  The stride of an axis
    of length 1 says nothing and is set to what the rows form wants."""
    if not isinstance(a, np.ndarray) or a.ndim != 2 or a.shape[0] == 0 or a.shape[1] == 0:
        return None
    code = VIEW_DTYPES.get(a.dtype) if a.dtype.isnative else None
    if code is None:
        return None
    n, d = a.shape
    size = a.dtype.itemsize
    if a.strides[0] % size or a.strides[1] % size:
        return None
    rs, cs = a.strides[0] // size, a.strides[1] // size
    if d == 1:
        cs = 1
    if n == 1:
        rs = d if cs == 1 else 1
    if not ((cs == 1 and rs >= d) or (rs == 1 and cs >= n)):
        return None
    return CcPointsView(a.ctypes.data, n, d, code, rs, cs)


def points_source(a):
    """(points, view): what the library takes of `a` with the fewest copies.  A C-contiguous 2-d float32 or float64 ndarray:
    (a, None) - the very object, for the entry points it has always taken.  An array points_view accepts: (a, its
    cc_points_view) - the very object again, read where it lies by the `_view` entry points.  Everything else - negative or
    zero strides, both strides beyond one element, int64 / uint64 / bool / object, another byte order, lists, no points -
    (as_points(a), None): a C-contiguous float64 copy."""
    if isinstance(a, np.ndarray) and a.ndim == 2 and a.flags["C_CONTIGUOUS"] and a.dtype in (np.float32, np.float64) \
            and a.dtype.isnative:
        return a, None
    view = points_view(a)
    if view is not None:
        return a, view
    return as_points(a), None


def xt_rows(d):
    """Rows of the resident points' dimension-major copy (cc_points_download_xt): the padded scan width for 9 <= d <= 64."""
    return scan_width(d, False, False)[0] if 8 < d <= 64 else d


def _ptr(a, typ=_dp):
    return None if a is None else a.ctypes.data_as(typ)


def comm_unique_id():
    """The 128-byte RCCL id rank 0 hands to the other ranks of a stream group (cc_comm_unique_id)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().cc_comm_unique_id(buf)
    if rc != 0:
        raise ChronoclustHipError("cc_comm_unique_id failed (%s): is librccl available?" % _ERRORS.get(rc, rc))
    return buf.raw


def comm_init_local(handles):
    """Makes the Handles of this process one group (rank = position): the in-process transport of the exact
    multi-GPU path.  Each handle must then be driven by its own host thread; collective calls block until every
    member has made them."""
    arr = (C.c_void_p * len(handles))(*[h._h for h in handles])
    rc = load().cc_comm_init_local(arr, len(handles))
    if rc != 0:
        raise ChronoclustHipError("cc_comm_init_local failed: %s" % _ERRORS.get(rc, rc))


def format_points_csv(values, first_id, label_idx, labels, threads=8, chunk=65536, out=None):
    """The body of cluster_points_D{t}.csv (app.py:357-360, DataFrame.to_csv(index=False)) as bytes: one line per row of
    `values` [n, d] - "<id>,<label>,<repr(float)>,..." -, ids counting from first_id, labels[label_idx[r]] as the label
    (already CSV-quoted where needed; index -1 = the last label).  Formatted by cc_format_points_csv in chunks on a few
    threads (ctypes releases the GIL).  With `out` (a binary file object) the chunks are written to it in order as they
    become ready - the threads format ahead of the writer, nothing is joined in memory - and the byte count is returned."""
    from concurrent.futures import ThreadPoolExecutor
    lib = load()
    values = _f64(values)
    if values.ndim != 2:
        raise ValueError("values must be a [n, d] array, got shape %r" % (values.shape,))
    n, d = values.shape
    label_idx = np.ascontiguousarray(label_idx, dtype=np.int32)
    if label_idx.shape != (n,):  # (the C side reads n entries: a short array would be read past its end)
        raise ValueError("label_idx must hold one entry per row: shape %r for %d rows" % (label_idx.shape, n))
    if len(labels) < 1:
        raise ValueError("labels must not be empty")
    enc = [s.encode() for s in labels]
    offs = np.zeros(len(enc) + 1, np.int32)
    offs[1:] = np.cumsum([len(e) for e in enc])
    blob = b"".join(enc)
    per_row = 25 + max(len(e) for e in enc) + 33 * d + 2

    def work(a):
        b = min(n, a + chunk)
        buf = np.empty(per_row * (b - a), np.uint8)  # (not zeroed: the formatter says how much of it it filled)
        got = lib.cc_format_points_csv(values[a:b].ctypes.data_as(_dp), b - a, d, first_id + a,
                                       label_idx[a:b].ctypes.data_as(_i32p), blob, offs.ctypes.data_as(_i32p), len(enc),
                                       buf.ctypes.data, buf.size)
        if got < 0:
            raise ChronoclustHipError("cc_format_points_csv failed: %s" % _ERRORS.get(got, got))
        return memoryview(buf)[:got]

    if n == 0:
        return 0 if out is not None else b""
    starts = list(range(0, n, chunk))
    workers = max(1, threads)
    with ThreadPoolExecutor(max_workers=workers) as ex:
        if out is None:
            return b"".join(ex.map(work, starts))
        # a bounded number of chunks in flight: the formatters run at most 2 x workers chunks ahead of the writer
        total, pending, nxt = 0, [], 0
        while nxt < len(starts) or pending:
            while nxt < len(starts) and len(pending) < 2 * workers:
                pending.append(ex.submit(work, starts[nxt]))
                nxt += 1
            part = pending.pop(0).result()
            out.write(part)
            total += len(part)
        return total


def policy_replay(config, carry, start, observations):
    """cc_policy_replay: the window policy over recorded observations, no GPU.  config: dict of cc_policy_config fields;
    carry: (adapt_win, clean_batches, since_shrink); start: (cursor, rows); observations: dicts of cc_policy_obs fields.
    Returns (decisions as dicts - one more than observations -, carry after the call)."""
    cfg = CcPolicyConfig(**{k: int(v) for k, v in config.items()})
    car = CcPolicyCarry(int(carry[0]), int(carry[1]), int(carry[2]), 0)
    n = len(observations)
    obs = (CcPolicyObs * max(n, 1))()
    for i, o in enumerate(observations):
        for k, v in o.items():
            if k == "round_hist":
                for r, x in enumerate(v):
                    obs[i].round_hist[r] = int(x)
            else:
                setattr(obs[i], k, int(v))
    out = (CcPolicyDecision * (n + 1))()
    rc = load().cc_policy_replay(C.byref(cfg), C.byref(car), int(start[0]), int(start[1]), obs, n, out)
    if rc != 0:
        raise ValueError("cc_policy_replay: %s" % _ERRORS.get(rc, rc))
    keys = [k for k, _ in CcPolicyDecision._fields_ if k != "pad"]
    return [{k: getattr(d, k) for k in keys} for d in out], (car.adapt_win, car.clean_batches, car.since_shrink)


def seq_handover_replay(mode, possible, sticky, events):
    """cc_seq_handover_replay: the hand-over rule between the windows and the sequential kernel (cc::SeqHandover) over
    events, no GPU and no clock.  events: dicts of cc_seq_event fields (chunk_event=1: a chunk of the sequential kernel, else a
    batch of windows).  Returns (outcomes, stint lengths), one entry more than events: [0] is the start of the call."""
    n = len(events)
    ev = (CcSeqEvent * max(n, 1))(*[CcSeqEvent(**e) for e in events])
    out, stint = (C.c_int32 * (n + 1))(), (C.c_int64 * (n + 1))()
    rc = load().cc_seq_handover_replay(int(mode), int(possible), int(sticky), ev, n, out, stint)
    if rc != 0:
        raise ValueError("cc_seq_handover_replay: %s" % _ERRORS.get(rc, rc))
    return list(out), list(stint)


def batch_plan(**inputs):
    """cc_batch_plan: the launch geometry of one batch of windows (cc::BatchPlan) from cc_batch_inputs fields, no GPU."""
    out = CcBatchGeometry()
    rc = load().cc_batch_plan(C.byref(CcBatchInputs(**inputs)), C.byref(out))
    if rc != 0:
        raise ValueError("cc_batch_plan(%r): %s" % (inputs, _ERRORS.get(rc, rc)))
    return {k: getattr(out, k) for k, _ in CcBatchGeometry._fields_ if k != "pad"}


SCAN_CHAINS = ("none", "common", "general")  # CC_CHAIN_*


def scan_width(d, filter_on, k_pow2):
    """cc_scan_width: (padded width, k_scan_u serves the plain scan, pruned chain - one of SCAN_CHAINS) for a stream of d
    dimensions with the pdim filter on or off and k a power of two or not, before any knob (cc::scan_width; no GPU needed)."""
    padded, scan_u, chain = C.c_int32(), C.c_int32(), C.c_int32()
    rc = load().cc_scan_width(int(d), int(bool(filter_on)), int(bool(k_pow2)), C.byref(padded), C.byref(scan_u), C.byref(chain))
    if rc != 0:
        raise ValueError("cc_scan_width(%r, %r, %r): %s" % (d, filter_on, k_pow2, _ERRORS.get(rc, rc)))
    return padded.value, bool(scan_u.value), SCAN_CHAINS[chain.value]


def shard_rows(n, world, rank, unit=1):
    """[lo, hi) of n rows for `rank` of `world` in units of `unit` rows (cc_shard_rows; no GPU needed)."""
    lo, hi = C.c_int32(), C.c_int32()
    rc = load().cc_shard_rows(int(n), int(world), int(rank), int(unit), C.byref(lo), C.byref(hi))
    if rc != 0:
        raise ValueError("cc_shard_rows(%r, %r, %r, %r): %s" % (n, world, rank, unit, _ERRORS.get(rc, rc)))
    return lo.value, hi.value


# The takers of points by kind of source (Handle._source): (operation, kind) -> C-ABI symbol.  A described source ("view",
# "list", "list_xf": a ListMode with a transform, "list_xl": one whose transform has a logicle row that is on) has one upload that
# takes scale / min_ or two nulls; rows have a plain and a scaled one.  "view_xl": a TransformedPoints.
_DESCRIBED = ("view", "view_xl", "list", "list_xf", "list_xl")
SOURCE_OBJECTS = (ListMode, TransformedPoints)  # what describes its own points: never copied, never handed to points_source
_INGEST = {
    "upload": {"f64": "cc_points_upload", "f32": "cc_points_upload_f32",
               "view": "cc_points_upload_view", "view_xl": "cc_points_upload_view_xl", "list": "cc_points_upload_list",
               "list_xf": "cc_points_upload_list_xf", "list_xl": "cc_points_upload_list_xl"},
    "upload_scaled": {"f64": "cc_points_upload_scaled", "f32": "cc_points_upload_scaled_f32",
                      "view": "cc_points_upload_view", "view_xl": "cc_points_upload_view_xl", "list": "cc_points_upload_list",
                      "list_xf": "cc_points_upload_list_xf", "list_xl": "cc_points_upload_list_xl"},
    "prefetch": {"f64": "cc_points_prefetch", "f32": "cc_points_prefetch_f32",
                 "view": "cc_points_prefetch_view", "view_xl": "cc_points_prefetch_view_xl", "list": "cc_points_prefetch_list",
                 "list_xf": "cc_points_prefetch_list_xf", "list_xl": "cc_points_prefetch_list_xl"},
    "col_minmax": {"f64": "cc_col_minmax", "f32": "cc_col_minmax_f32",
                   "view": "cc_col_minmax_view", "view_xl": "cc_col_minmax_view_xl", "list": "cc_col_minmax_list",
                   "list_xf": "cc_col_minmax_list_xf", "list_xl": "cc_col_minmax_list_xl"},
    "assign": {"f64": "cc_assign", "f32": "cc_assign_f32", "view": "cc_assign_view", "view_xl": "cc_assign_view_xl", "list": "cc_assign_list",
               "list_xf": "cc_assign_list_xf", "list_xl": "cc_assign_list_xl"},
}
_SCALED_REFUSAL = "points must be [n, d], scale and min_ [d]"


class Handle(object):
    """One HDDStream state on one GPU."""

    def __init__(self, device=0):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.cc_create(int(device), C.byref(h))
        if rc != 0:
            raise ChronoclustHipError("cc_create(device=%d) failed: %s. chronoclust_amd needs an MI355X-class HIP "
                                      "device; there is no CPU fallback." % (device, _ERRORS.get(rc, rc)))
        self._h = h
        self.device = device
        self._prefetched = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            msg = self._lib.cc_last_error(self._h)
            exc = ValueError if rc in (-2, -3) else ChronoclustHipError
            raise exc("%s: %s" % (_ERRORS.get(rc, rc), msg.decode() if msg else ""))
        return rc

    def set_tuning(self, window=0, rounds=0, segments=0, windows_per_sync=0, time_kernels=0, dirty_segments=0,
                   lookahead=0, early_window=0, sequential=0):
        t = CcTuning(window, rounds, segments, windows_per_sync, time_kernels, dirty_segments, int(early_window),
                     int(lookahead), int(sequential))
        self._check(self._lib.cc_set_tuning(self._h, C.byref(t)))

    def reset(self):
        self._check(self._lib.cc_reset(self._h))

    def set_params(self, eps_sq, delta_sq, k, beta, mu, omicron, ups_eps, ups_eps_sq, delta, pi):
        p = CcParams(eps_sq, delta_sq, k, beta, mu, omicron, ups_eps, ups_eps_sq, delta, int(pi), 0)
        self._check(self._lib.cc_set_params(self._h, C.byref(p)))

    def decay_downgrade(self, factor):
        self._check(self._lib.cc_decay_downgrade(self._h, float(factor)))

    def _source(self, x, refusal="points must be a 2-d array"):
        """(kind, points, args, n, d) of what a taker of points is given: the kind of source - "list" (a ListMode; "list_xf"
        with a transform, "list_xl" with a logicle row that is on), "view_xl" (a TransformedPoints), "view"
        (an array points_view accepts), "f32" or "f64" (C-contiguous rows; everything else as a float64 copy: points_source) -,
        the object that owns the memory, and the C arguments that describe it: (descriptor,) or (pointer, n, d)."""
        if isinstance(x, ListMode):
            desc, xf, lg = x.descriptor(), x.transform_descriptor(), x.logicle_descriptor()
            if lg is not None:
                return ("list_xl", x, (C.byref(desc), C.byref(xf), C.byref(lg))) + x.shape
            if xf is not None:
                return ("list_xf", x, (C.byref(desc), C.byref(xf))) + x.shape
            return ("list", x, (C.byref(desc),)) + x.shape
        if isinstance(x, TransformedPoints):
            # (the array where it lies, or the object's own float64 copy; the library takes a null transform or null rows)
            view, xf, lg = x.descriptor(), x.transform_descriptor(), x.logicle_descriptor()
            return ("view_xl", x, (C.byref(view), None if xf is None else C.byref(xf), None if lg is None else C.byref(lg))) + x.shape
        x, view = points_source(x)
        if x.ndim != 2:
            raise ValueError(refusal)
        if view is not None:
            return ("view", x, (C.byref(view),)) + x.shape
        f32 = x.dtype == np.float32
        return ("f32" if f32 else "f64", x, (_ptr(x, _fp if f32 else _dp),) + x.shape) + x.shape

    def _ingest(self, op, kind, *args):
        self._check(getattr(self._lib, _INGEST[op][kind])(self._h, *args))

    def _upload(self, x, scale, min_):
        kind, x, args, n, d = self._source(x, "points must be a 2-d array" if scale is None else _SCALED_REFUSAL)
        op = "upload"
        if scale is not None:
            op, scale, min_ = "upload_scaled", _f64(scale), _f64(min_)
            if scale.shape != (d,) or min_.shape != (d,):
                raise ValueError(_SCALED_REFUSAL)
        if scale is not None or kind in _DESCRIBED:  # (a descriptor's upload takes scale / min_ or two nulls)
            args += (_ptr(scale), _ptr(min_))
        try:
            self._ingest(op, kind, *args)
        finally:
            self._prefetched = None  # adopted or discarded by the library: the array is no longer pinned by us
        self._n = n

    def points_upload(self, x):
        self._upload(x, None, None)

    def points_upload_scaled(self, x, scale, min_):
        """points_upload of x * scale + min_ (MinMaxScaler.transform), scaled on the device."""
        self._upload(x, scale, min_)

    def points_prefetch(self, x, scale=None, min_=None):
        """Starts the background upload of the NEXT timepoint's points (cc_points_prefetch).  `x` must be the very
        array (C-contiguous float64 or float32, or one points_view accepts), ListMode or TransformedPoints that is later passed to points_upload /
        points_upload_scaled / online; the handle keeps a reference to it until then.  Contract: the array must not be
        written to between this call and that upload - the upload is recognised by pointer, shape, layout, element type and
        scaling, and the copy already on the device is used as it is."""
        if isinstance(x, (np.ndarray,) + SOURCE_OBJECTS) and x.ndim == 2 and x.shape[0] == 0:
            return
        refusal = ("points_prefetch needs an [n, d] array that is taken as it lies - C-contiguous float64 or float32, "
                   "or a layout and element type points_view accepts (it is not copied)")
        kind, src, args, n, d = self._source(x, refusal)
        if src is not x:
            raise ValueError(refusal)
        scale = None if scale is None else _f64(scale)
        min_ = None if min_ is None else _f64(min_)
        self._prefetched = (x, scale, min_)  # keeps the buffers alive while the worker reads them
        self._ingest("prefetch", kind, *(args + (_ptr(scale), _ptr(min_))))

    def col_minmax(self, x):
        """Per-column (min, max) of x, NaN ignored, reduced on the device."""
        kind, x, args, n, d = self._source(x)
        mn = np.empty(d, dtype=np.float64)
        mx = np.empty(d, dtype=np.float64)
        self._ingest("col_minmax", kind, *(args + (_ptr(mn), _ptr(mx))))
        return mn, mx

    def negative_quantiles(self, sources, q=0.05, want=None):
        """(count, lo, hi, frac), each [d]: per selected dimension the exact order statistics around quantile q of the NEGATIVE
        compensated values of `sources` - a list of ListMode of one width, pooled; each carries its own compensation in its
        ListTransform, whose cofactors and logicle rows are ignored -, selected on the device (cc_negq_begin / _add_list /
        _select / _end).  count = the negative values (NaN, +-0 and positive values are none; -Inf is), h = (count - 1) * q,
        j = floor(h), frac = h - j, lo = sorted[j], hi = sorted[min(j + 1, count - 1)], bit for bit; count == 0: zeros.
        np.quantile(np.array([lo, hi]), frac) is np.quantile of the negative values at q.  want: a mask [d] of the dimensions to
        select (None: all); the others come back with count -1 and zeros.  Nothing else of the handle changes."""
        sources, d, want = _negq_sources(sources, want)
        count = np.empty(d, np.int64)
        lo, hi, frac = np.empty(d), np.empty(d), np.empty(d)
        self._check(self._lib.cc_negq_begin(self._h, d, _ptr(want, C.POINTER(C.c_uint8)), sum(s.n for s in sources)))
        try:
            for s in sources:
                if s.n == 0:
                    continue  # (an empty DATA segment has no address to describe)
                desc, t = s.descriptor(), s.transform
                xf = None
                if t is not None and t.m:
                    xf = C.byref(CcListTransform(t.m, 0, t.comp_cols.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 t.comp.ctypes.data_as(C.POINTER(C.c_double)), None))
                self._check(self._lib.cc_negq_add_list(self._h, C.byref(desc), xf))
            self._check(self._lib.cc_negq_select(self._h, float(q), _ptr(count, _i64p), _ptr(lo), _ptr(hi), _ptr(frac)))
        finally:
            self._lib.cc_negq_end(self._h)
        return count, lo, hi, frac

    def points_download(self, d, scale=None, min_=None):
        """The resident points; with scale / min_, (X - min_) / scale (MinMaxScaler.inverse_transform)."""
        out = np.empty((self._n, d), dtype=np.float64)
        if scale is None:
            self._check(self._lib.cc_points_download(self._h, _ptr(out), None, None))
        else:
            scale, min_ = _f64(scale), _f64(min_)
            self._check(self._lib.cc_points_download(self._h, _ptr(out), _ptr(scale), _ptr(min_)))
        return out

    def points_download_xt(self, d):
        """The resident points' dimension-major copy as the scans read it: [xt_rows(d), n], the padded rows +0.0."""
        out = np.empty((xt_rows(d), self._n), dtype=np.float64)
        self._check(self._lib.cc_points_download_xt(self._h, _ptr(out)))
        return out

    def online_run(self):
        self._check(self._lib.cc_online_run(self._h))

    def labels_download(self, want_path=True):
        uid = np.empty(self._n, dtype=np.int64)
        path = np.empty(self._n, dtype=np.int8) if want_path else None
        self._check(self._lib.cc_labels_download(self._h, _ptr(uid, _i64p), _ptr(path, _i8p)))
        return uid, path

    def online(self, x):
        self.points_upload(x)
        self.online_run()
        return self.labels_download()

    def assign(self, x, want_path=True, want_dist=False):
        """cc_assign: per point of x [n, d] what the online phase would do with it if it were the very next point, against
        the table as it stands - (uid, path, dist): the creation number of the microcluster it would join (-1: it would
        create one), 0 pcore / 1 outlier / 5 outlier that the add promotes / 2 new, the projected distance to that
        microcluster (-1.0 for path 2); path and dist are None unless wanted.  Nothing of the handle changes."""
        kind, x, args, n, d = self._source(x)
        uid = np.empty(n, dtype=np.int64)
        path = np.empty(n, dtype=np.int8) if want_path else None
        dist = np.empty(n, dtype=np.float64) if want_dist else None
        self._ingest("assign", kind, *(args + (_ptr(uid, _i64p), _ptr(path, _i8p), _ptr(dist))))
        return uid, path, dist

    def count(self, kind):
        return self._check(self._lib.cc_count(self._h, kind))

    def dim(self):
        return self._check(self._lib.cc_dim(self._h))

    def counters(self):
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.cc_counters(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_counters(self, pcore_last_id, outlier_last_id):
        self._check(self._lib.cc_set_counters(self._h, int(pcore_last_id), int(outlier_last_id)))

    def export(self, kind):
        n, d = self.count(kind), self.dim()
        out = dict(id=np.empty(n, np.int64), uid=np.empty(n, np.int64), w=np.empty(n, np.float64),
                   cf1=np.empty((n, d)), cf2=np.empty((n, d)), cen=np.empty((n, d)), pref=np.empty((n, d)))
        self._check(self._lib.cc_export(self._h, kind, _ptr(out["id"], _i64p), _ptr(out["uid"], _i64p), _ptr(out["w"]),
                                        _ptr(out["cf1"]), _ptr(out["cf2"]), _ptr(out["cen"]), _ptr(out["pref"])))
        return out

    def inject(self, kind, cf1, cf2, cen, pref, w, id, uid):
        cf1, cf2, cen, pref = _f64(cf1), _f64(cf2), _f64(cen), _f64(pref)
        self._check(self._lib.cc_inject_mc(self._h, kind, len(cf1), _ptr(cf1), _ptr(cf2), _ptr(cen), _ptr(pref),
                                           float(w), int(id), int(uid)))

    def inject_bulk(self, kind, cf1, cf2, cen, pref, w, id, uid):
        """Appends len(w) microclusters to a list with one upload per column (cc_inject_bulk)."""
        cf1, cf2, cen, pref, w = _f64(cf1), _f64(cf2), _f64(cen), _f64(pref), _f64(w)
        id = np.ascontiguousarray(id, dtype=np.int64)
        uid = np.ascontiguousarray(uid, dtype=np.int64)
        n = w.shape[0]
        if n == 0:
            return
        if cf1.shape != (n, cf1.shape[1]) or any(a.shape != cf1.shape for a in (cf2, cen, pref)) or \
                id.shape != (n,) or uid.shape != (n,):
            raise ValueError("inject_bulk: cf1/cf2/cen/pref must be [n, d], w/id/uid [n]")
        self._check(self._lib.cc_inject_bulk(self._h, kind, cf1.shape[1], n, _ptr(cf1), _ptr(cf2), _ptr(cen),
                                             _ptr(pref), _ptr(w), _ptr(id, _i64p), _ptr(uid, _i64p)))

    def offline_arrays(self, dumps=False):
        """cc_offline + cc_clusters_export: (members, offsets, w, cf1, cf2, cen, pref), info - all clusters as arrays."""
        n = C.c_int32()
        m = self.count(PCORE) if dumps else 0
        core = np.zeros(m, np.int8) if dumps else None
        pdim, nn, nw = ((np.zeros(m, np.int32) for _ in range(3)) if dumps else (None, None, None))
        self._check(self._lib.cc_offline(self._h, C.byref(n), _ptr(core, _i8p), _ptr(pdim, _i32p), _ptr(nn, _i32p),
                                         _ptr(nw, _i32p)))
        d, nc = self.dim(), n.value
        tot = self._check(self._lib.cc_clusters_total_members(self._h))
        mem = np.empty(tot, np.int64)
        off = np.zeros(nc + 1, np.int32)
        w = np.empty(nc, np.float64)
        cf1, cf2, cen, pref = (np.empty((nc, d)) for _ in range(4))
        self._check(self._lib.cc_clusters_export(self._h, _ptr(mem, _i64p), _ptr(off, _i32p), _ptr(w), _ptr(cf1),
                                                 _ptr(cf2), _ptr(cen), _ptr(pref)))
        info = dict(core=core, pdim=pdim, nn=nn, nw=nw) if dumps else None
        return (mem, off, w, cf1, cf2, cen, pref), info

    def offline(self, dumps=False):
        """The same, one dict per cluster."""
        (mem, off, w, cf1, cf2, cen, pref), info = self.offline_arrays(dumps)
        clusters = [dict(members=mem[off[c]:off[c + 1]], w=float(w[c]), cf1=cf1[c], cf2=cf2[c], cen=cen[c],
                         pref=pref[c]) for c in range(len(w))]
        return clusters, info

    def point_clusters(self):
        """Cluster index (order of offline_arrays) of every resident point, -1 outside every cluster (cc_point_clusters)."""
        out = np.empty(self._n, dtype=np.int32)
        if self._n:
            self._check(self._lib.cc_point_clusters(self._h, _ptr(out, _i32p)))
        return out

    def num_core(self):
        return self._check(self._lib.cc_num_core(self._h))

    def assoc_argmin(self, cur_cen, cur_pref, prev_cen):
        cc, cp, pc = _f64(cur_cen), _f64(cur_pref), _f64(prev_cen)
        mc, d = cc.shape
        mp = pc.shape[0]
        idx = np.empty(mc, np.int32)
        dist = np.empty(mc, np.float64)
        self._check(self._lib.cc_assoc_argmin(self._h, _ptr(cc), _ptr(cp), mc, _ptr(pc), mp, d, _ptr(idx, _i32p),
                                              _ptr(dist)))
        return idx, dist

    def comm_init_rccl(self, unique_id, rank, world):
        """Joins the RCCL communicator of a stream group (collective over the `world` processes)."""
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique_id must be %d bytes" % COMM_ID_BYTES)
        self._check(self._lib.cc_comm_init_rccl(self._h, bytes(unique_id), int(rank), int(world)))

    def comm_calibrate(self):
        """Measures the all-gather of a window's records and a plain scan and derives the split thresholds from them
        (cc_comm_calibrate; collective: every rank of the group calls it - the members of an in-process group from their
        own threads; cc_comm_init_rccl has done it already).  Returns the measured figures and the thresholds."""
        self._check(self._lib.cc_comm_calibrate(self._h))
        s = self.stats()
        return {k: s[k] for k in ("calib_allgather_us", "calib_scan_ns_per_row_dim", "split_threshold_row_dims",
                                  "split_threshold_row_dims_pruned")}

    def comm_destroy(self):
        self._check(self._lib.cc_comm_destroy(self._h))

    def comm_info(self):
        r, w, t = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.cc_comm_info(self._h, C.byref(r), C.byref(w), C.byref(t)))
        return dict(rank=r.value, world=w.value, transport={0: "none", 1: "rccl", 2: "local"}[t.value])

    def comm_set_relaxed(self, minibatch_points):
        """RELAXED multi-GPU mode (events sharded over the ranks, CF deltas all-reduced per super-step of
        `minibatch_points` points per rank; not the reference's semantics).  0: back to the exact path."""
        self._check(self._lib.cc_comm_set_relaxed(self._h, int(minibatch_points)))

    def relaxed_stats(self):
        s = CcRelaxedStats()
        self._check(self._lib.cc_get_relaxed_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in CcRelaxedStats._fields_ if k != "reserved"}

    def set_shard_thresholds(self, min_row_dims=-1, offline_min_rows=-1):
        self._check(self._lib.cc_set_shard_thresholds(self._h, int(min_row_dims), int(offline_min_rows)))

    def sync(self):
        """Waits for everything enqueued on the handle's HIP streams (cc_sync): the timing bracket of bench.py."""
        self._check(self._lib.cc_sync(self._h))

    def stats(self):
        s = CcStats()
        self._check(self._lib.cc_get_stats(self._h, C.byref(s)))
        out = {k: getattr(s, k) for k, _ in CcStats._fields_ if k != "reserved"}
        out["f32_points"] = self.f32_points()
        out["view_points"] = self.view_points()
        out["list_points"] = self.list_points()
        return out

    def f32_points(self):
        """Points this handle has taken in single precision since it was created (cc_f32_points): uploads, adopted
        prefetches and assigns of float32 arrays.  stats() carries it as "f32_points" beside the fields of cc_stats."""
        n = C.c_int64()
        self._check(self._lib.cc_f32_points(self._h, C.byref(n)))
        return n.value

    def list_points(self):
        """Events this handle has taken through the `_list` entry points since it was created (cc_list_points): uploads,
        adopted prefetches and assigns of ListMode records.  stats() carries it as "list_points"."""
        n = C.c_int64()
        self._check(self._lib.cc_list_points(self._h, C.byref(n)))
        return n.value

    def view_points(self):
        """Points this handle has taken through the `_view` entry points since it was created (cc_view_points): uploads,
        adopted prefetches and assigns of arrays read where they lie.  stats() carries it as "view_points"."""
        n = C.c_int64()
        self._check(self._lib.cc_view_points(self._h, C.byref(n)))
        return n.value
