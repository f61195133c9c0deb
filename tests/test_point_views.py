"""Point views end to end (cc_points_upload_view and its kin, k_ingest): what the device holds after an array went in where
it lies - column-major, pitched, narrow-typed - is, bit for bit, what it holds after the same values were widened and laid
out on the host and went in as C-contiguous float64: the row-major copy, the dimension-major copy with its padded rows, the
flag words; so labels, tables, clusters and every counter of the online phase, the answers of the read-only assignment, the
scaler's fit and the files app.run writes are the same.  The expectation is always the float64 route fed
np.ascontiguousarray(np.asarray(a, np.float64)); every comparison is of bit patterns, nothing is tolerated.  Shapes: the
smallest that cross a point tile (64), a block of dimensions (64), a padded scan width, a slab
(CHRONOCLUST_HIP_INGEST_SLAB=128: 300 points are three slabs, the last partial) and a chunk of cc_assign."""
import ctypes
import os

import numpy as np
import pytest

import assign_util as A
import scenarios
import table_util as T
from pipeline_util import knobs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

NS = (1, 63, 64, 65, 129, 300)
DS = (1, 3, 8, 9, 13, 20, 63, 64, 65, 130)
SLABS = (None, 128)
NARROW = (np.float16, np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32)
TIME_FIELDS = ("scan_ms", "run_ms", "comm_ms", "scan_ms_pruned", "calib_allgather_us", "calib_scan_ns_per_row_dim")


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float64
    return a.view(np.int64)


def same_bits(got, exp, what):
    diff = None if np.array_equal(bits(got), bits(exp)) else T._first_diff(bits(got), bits(exp))
    assert diff is None, "%s: %s" % (what, diff)


def widened(a):
    """What the float64 route is fed: the referee's input."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def specials(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        f = np.finfo(dtype)
        return np.array([0.0, -0.0, f.smallest_subnormal, -f.smallest_subnormal, np.nextafter(f.tiny, dtype.type(0)), f.tiny,
                         f.max, -f.max], dtype=dtype)  # (float16: 65504 the largest finite, 2^-24 the smallest subnormal)
    i = np.iinfo(dtype)
    return np.array([0, 1, i.max, i.min, i.max - 1, i.min + 1], dtype=dtype)  # (UINT32_MAX, INT32_MIN among them)


def values(dtype, n, d, turn=0):
    """Random [n, d] of the type with a special value at element 0, at the last element and at the last element of the first
    point tile - which one: by `turn` - and all of them scattered over the rest where there is room."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(1000 * n + d + dtype.itemsize)
    if dtype.kind == "f":
        x = rng.uniform(-4.0, 4.0, (n, d)).astype(dtype)
    else:
        i = np.iinfo(dtype)
        x = rng.integers(i.min, i.max, (n, d), dtype=dtype, endpoint=True)
    sp = specials(dtype)
    flat = x.reshape(-1)
    if flat.size > 40:
        flat[rng.choice(np.arange(1, flat.size - 1), 3 * len(sp), replace=False)] = np.tile(sp, 3)
    for k, at in enumerate((0, flat.size - 1, min(n, 64) * d - 1)):
        flat[at] = sp[(turn + k) % len(sp)]
    return x


def gap(dtype):
    """What lies between the rows or the strips of a pitched view: never read - NaN where the type has one."""
    return np.nan if np.dtype(dtype).kind == "f" else 77


def c_pitched(x, extra=5, first=2):
    n, d = x.shape
    big = np.full((n, d + extra), gap(x.dtype), dtype=x.dtype)
    big[:, first:first + d] = x
    return big[:, first:first + d]


def f_pitched(x):
    n, d = x.shape
    big = np.full((n + 7, d), gap(x.dtype), dtype=x.dtype, order="F")
    big[3:3 + n] = x
    return big[3:3 + n]


def every_other_row(x):
    n, d = x.shape
    big = np.full((2 * n, d), gap(x.dtype), dtype=x.dtype)
    big[::2] = x
    return big[::2]


# name -> the same values in that layout.  "C wide pitch": d of 9 d + 2 columns, beyond the pitch that travels whole
LAYOUTS = {
    "C pitched": c_pitched,
    "Fortran dense": np.asfortranarray,
    "Fortran pitched": f_pitched,
    "transpose of [d, N]": lambda x: np.ascontiguousarray(x.T).T,
    "every other row": every_other_row,
    "C wide pitch": lambda x: c_pitched(x, extra=8 * x.shape[1] + 2, first=1),
}


def raw_view(a, row_stride=None, col_stride=None, dtype=None, n=None, d=None):
    """A descriptor built by hand (the C level: no points_source in between)."""
    from chronoclust_amd import _lib
    size = a.dtype.itemsize
    return _lib.CcPointsView(a.ctypes.data, a.shape[0] if n is None else n, a.shape[1] if d is None else d,
                             _lib.VIEW_DTYPES[a.dtype] if dtype is None else dtype,
                             a.strides[0] // size if row_stride is None else row_stride,
                             a.strides[1] // size if col_stride is None else col_stride)


def upload_raw(h, a, view=None):
    """cc_points_upload_view of a descriptor, straight through ctypes."""
    view = raw_view(a) if view is None else view
    rc = h._lib.cc_points_upload_view(h._h, ctypes.byref(view), None, None)
    h._check(rc)
    h._n = a.shape[0]


@pytest.fixture(scope="module", params=SLABS, ids=lambda s: "slab%s" % s)
def handle(request):
    """One handle per slab setting for the tests that only move points (the knob is read when a handle is created)."""
    from chronoclust_amd import _lib
    env = {} if request.param is None else dict(CHRONOCLUST_HIP_INGEST_SLAB=request.param)
    with knobs(**env):
        h = _lib.Handle(0)
    yield h
    h.close()


def resident(h, d):
    return h.points_download(d), h.points_download_xt(d)


def referee(h, wide, scaling=None):
    """The float64 route on the widened dense array: (row-major copy, dimension-major copy)."""
    from chronoclust_amd import _lib
    n, d = wide.shape
    before = h.stats()
    if scaling is None:
        h.points_upload(wide)
    else:
        h.points_upload_scaled(wide, *scaling)
    after = h.stats()
    assert after["view_points"] == before["view_points"] and after["f32_points"] == before["f32_points"]
    x, xt = resident(h, d)
    assert xt.shape == (_lib.xt_rows(d), n) and not bits(xt[d:]).any()
    same_bits(xt[:d], x.T, "the referee's own two copies")
    return x, xt


def check_view(h, a, exp, what, scaling=None, raw=False):
    """`a` goes in as it lies; the two resident copies are the referee's, and the counters say which route it took."""
    from chronoclust_amd import _lib
    n, d = a.shape
    src, view = _lib.points_source(a)
    assert raw or (src is a and view is not None), what + ": not taken as it lies"
    before = h.stats()
    if raw:
        upload_raw(h, a)
    elif scaling is None:
        h.points_upload(a)
    else:
        h.points_upload_scaled(a, *scaling)
    after = h.stats()
    assert after["view_points"] == before["view_points"] + n, what
    assert after["f32_points"] == before["f32_points"], what
    x, xt = resident(h, d)
    same_bits(x, exp[0], what + " row-major")
    assert xt.shape == exp[1].shape, what
    same_bits(xt, exp[1], what + " dimension-major with its pad rows")


# ---- 1. ingest alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
def test_ingest_alone(handle, n):
    for i, d in enumerate(DS):
        for dtype in (np.float64, np.float32):
            x = values(dtype, n, d, turn=NS.index(n) + i)
            wide = widened(x)
            exp = referee(handle, wide)
            same_bits(exp[0], wide, "the referee holds the widened values")
            check_view(handle, x, exp, "%s C dense %d x %d" % (np.dtype(dtype).name, n, d), raw=True)
            for name, lay in LAYOUTS.items():
                if name == "C wide pitch" and d > 20:
                    continue
                a = lay(x)
                assert widened(a).tobytes() == wide.tobytes()
                if (n == 1 or d == 1) and a.flags["C_CONTIGUOUS"]:
                    continue  # (one strip or one row: the array is C-contiguous too and takes the entry points of old)
                check_view(handle, a, exp, "%s %s %d x %d" % (np.dtype(dtype).name, name, n, d))


@pytest.mark.parametrize("dtype", NARROW, ids=lambda t: np.dtype(t).name)
def test_ingest_narrow_types(handle, dtype):
    for i, (n, d) in enumerate([(1, 1), (1, 9), (65, 1), (65, 9), (65, 20), (300, 13), (300, 65), (129, 130)]):
        x = values(dtype, n, d, turn=i)
        exp = referee(handle, widened(x))
        for name in ("C pitched", "Fortran pitched", "C wide pitch"):
            if name == "C wide pitch" and d > 20:
                continue
            check_view(handle, LAYOUTS[name](x), exp, "%s %s %d x %d" % (np.dtype(dtype).name, name, n, d))
        check_view(handle, x, exp, "%s C dense %d x %d" % (np.dtype(dtype).name, n, d))


def test_ingest_1024_dimensions(handle):
    for dtype in (np.float64, np.float32, np.uint16):
        x = values(dtype, 70, 1024, turn=3)
        exp = referee(handle, widened(x))
        for name in ("C pitched", "Fortran pitched"):
            check_view(handle, LAYOUTS[name](x), exp, "%s %s 70 x 1024" % (np.dtype(dtype).name, name))


# ---- 2. scaled ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d", [(1, 3), (65, 13), (129, 20), (300, 9), (129, 130)])
def test_scaled(handle, n, d):
    from chronoclust_amd.scaling.scaler import Scaler
    for dtype in (np.float32, np.float64, np.uint16):
        x = values(dtype, n, d, turn=n + d)
        if np.dtype(dtype).kind == "f":
            x = np.clip(x, -1e30, 1e30).astype(dtype)  # (a range whose reciprocal is a normal number)
        wide = widened(x)
        sc = Scaler()
        sc.fit_scaler(wide)
        scaling = (sc.scale_, sc.min_)
        exp = referee(handle, wide, scaling)
        same_bits(exp[0], wide * sc.scale_ + sc.min_, "the referee holds numpy's two roundings")
        for name in ("C pitched", "Fortran pitched"):
            a = LAYOUTS[name](x)
            if n == 1 and a.flags["C_CONTIGUOUS"] and a.dtype != np.uint16:
                continue  # (one row: C-contiguous too, the entry points of old)
            check_view(handle, a, exp, "scaled %s %s %d x %d" % (np.dtype(dtype).name, name, n, d), scaling=scaling)


def test_a_scale_that_overflows_is_refused_as_on_the_float64_route(handle):
    x32 = np.random.default_rng(5).uniform(1.0, 2.0, (300, 5)).astype(np.float32)
    x32[200, 3] = 1e30
    x16 = np.random.default_rng(6).integers(1, 60000, (300, 5)).astype(np.uint16)
    for x in (x32, x16):
        scale, min_ = np.ones(5), np.zeros(5)
        for a in (widened(x), c_pitched(x), f_pitched(x)):
            handle.points_upload_scaled(a, scale, min_)  # finite as long as the scale leaves it so
        scale[3] = 1e305
        for a in (widened(x), c_pitched(x), f_pitched(x)):
            with pytest.raises(ValueError, match="non-finite"):
                handle.points_upload_scaled(a, scale, min_)


# ---- 3. non-finite input ----------------------------------------------------------------------------------------------------

def test_non_finite_input_is_refused_and_leaves_the_handle_sound():
    """300 points in slabs of 128: element 0, the last element, the last partial tile (points 256 ..) and a later slab; a
    float64 Fortran-order array and a float16 C-pitched one; from the upload, from a prefetch followed by the upload and from
    assign.  Afterwards the handle clusters a clean array exactly as a fresh handle does."""
    from chronoclust_amd import _lib
    name = "stale-31+33x5"
    pcores, outliers, par, X = A.case(name)[:4]
    clean16 = np.tile(X, (3, 1))[:300].astype(np.float16)
    n, d = clean16.shape
    makers = (lambda v: np.asfortranarray(v.astype(np.float64)), lambda v: c_pitched(v))

    def online(h, x):
        T.fill_handle(h, par, pcores, outliers)
        h.set_tuning(sequential=1)
        labels = h.online(x)
        return labels, [h.export(kind) for kind in (_lib.PCORE, _lib.OUTLIER)], h.counters()

    with knobs(CHRONOCLUST_HIP_INGEST_SLAB=128, CHRONOCLUST_HIP_ASSIGN_CHUNK=128):
        h, fresh = _lib.Handle(0), _lib.Handle(0)
    try:
        T.fill_handle(h, par, pcores, outliers)
        for make in makers:
            for value in (np.nan, np.inf, -np.inf):
                for at in ((0, 0), (n - 1, d - 1), (270, 2), (200, 1)):
                    bad = clean16.copy()
                    bad[at] = value
                    bad = make(bad)
                    assert _lib.points_source(bad)[1] is not None
                    with pytest.raises(ValueError, match="non-finite"):
                        h.points_upload(bad)
                    h.points_prefetch(bad)
                    with pytest.raises(ValueError, match="non-finite"):
                        h.points_upload(bad)
                    with pytest.raises(ValueError, match="non-finite"):
                        h.assign(bad)
        exp = online(fresh, widened(clean16))
        for make in makers:
            h.reset()
            got = online(h, make(clean16))
            for key, a, b in (("uid", got[0][0], exp[0][0]), ("path", got[0][1], exp[0][1])):
                assert T._first_diff(a, b) is None, (key, T._first_diff(a, b))
            for kind in (0, 1):
                for key in T.KEYS:
                    assert got[1][kind][key].tobytes() == exp[1][kind][key].tobytes(), (kind, key)
            assert got[2] == exp[2]
    finally:
        h.close()
        fresh.close()


# ---- 4. descriptor refusals at the C level -----------------------------------------------------------------------------------

def test_descriptor_refusals(handle):
    from chronoclust_amd import _lib
    a = values(np.float64, 40, 6)
    wide1025 = np.zeros((2, 1025))
    cases = [("both strides 2", raw_view(a, row_stride=2, col_stride=2, n=10, d=3)),
             ("a zero stride", raw_view(a, row_stride=0, col_stride=1)),
             ("a zero column stride", raw_view(a, row_stride=1, col_stride=0)),
             ("a negative stride", raw_view(a, row_stride=-6, col_stride=1)),
             ("dtype 99", raw_view(a, dtype=99)),
             ("d = 1025", raw_view(wide1025)),
             ("rows that overlap", raw_view(a, row_stride=3, col_stride=1)),
             ("an extent beyond int64", raw_view(a, row_stride=2 ** 62, col_stride=1))]
    exp = referee(handle, a)
    before = handle.stats()
    mn, mx = np.zeros(1025), np.zeros(1025)
    uid, path = np.zeros(40, np.int64), np.zeros(40, np.int8)
    lib, hh = handle._lib, handle._h
    for what, view in cases:
        calls = [lib.cc_points_upload_view(hh, ctypes.byref(view), None, None),
                 lib.cc_points_prefetch_view(hh, ctypes.byref(view), None, None),
                 lib.cc_col_minmax_view(hh, ctypes.byref(view), _lib._ptr(mn), _lib._ptr(mx)),
                 lib.cc_online_view(hh, ctypes.byref(view), _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p)),
                 lib.cc_assign_view(hh, ctypes.byref(view), _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p), None)]
        assert calls == [-2] * 5, (what, calls)  # CC_ERR_BAD_ARG
        assert len(lib.cc_last_error(hh)) > 10, what
        with pytest.raises(ValueError, match="bad argument"):
            handle._check(calls[0])
    # scale without min_
    ok = raw_view(a)
    assert lib.cc_points_upload_view(hh, ctypes.byref(ok), _lib._ptr(mn), None) == -2
    # nothing moved: the resident points are the referee's, no point was counted
    assert handle.stats()["view_points"] == before["view_points"]
    x, xt = resident(handle, 6)
    same_bits(x, exp[0], "resident points behind refused calls")
    check_view(handle, np.asfortranarray(a), exp, "a good view behind refused ones")
    # the stride of an axis of length 1 says nothing: one dimension or one point is taken whatever it is
    col = np.ascontiguousarray(a[:, :1])
    one = np.ascontiguousarray(a[:1])
    for what, arr, view in (("d = 1, column stride 3", col, raw_view(col, row_stride=1, col_stride=3)),
                            ("d = 1, column stride 2^40", col, raw_view(col, row_stride=1, col_stride=2 ** 40)),
                            ("n = 1, row stride 2", one, raw_view(one, row_stride=2, col_stride=1)),
                            ("n = 1, row stride 2^40", one, raw_view(one, row_stride=2 ** 40, col_stride=1))):
        upload_raw(handle, arr, view)
        same_bits(handle.points_download(arr.shape[1]), arr, what)


def test_online_and_assign_views_at_the_c_level():
    """cc_online_view and cc_assign_view straight through ctypes (the Python layer uploads, runs and downloads in three calls)."""
    from chronoclust_amd import _lib
    name = "stale-31+33x5"
    pcores, outliers, par, X = A.case(name)[:4]
    xf = np.asfortranarray(X)
    n = len(X)
    h, fresh = _lib.Handle(0), _lib.Handle(0)
    try:
        for g in (h, fresh):
            T.fill_handle(g, par, pcores, outliers)
        exp_assign = fresh.assign(widened(X), want_dist=True)
        exp = fresh.online(widened(X))
        view = raw_view(xf)
        uid, path, dist = np.empty(n, np.int64), np.empty(n, np.int8), np.empty(n, np.float64)
        h._check(h._lib.cc_assign_view(h._h, ctypes.byref(view), _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p), _lib._ptr(dist)))
        A.same_assign((uid, path, dist), exp_assign, name + " cc_assign_view")
        uid, path = np.empty(n, np.int64), np.empty(n, np.int8)
        h._check(h._lib.cc_online_view(h._h, ctypes.byref(view), _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p)))
        assert T._first_diff(uid, exp[0]) is None and T._first_diff(path, exp[1]) is None
        for kind in (0, 1):
            got, want = h.export(kind), fresh.export(kind)
            for key in T.KEYS:
                assert got[key].tobytes() == want[key].tobytes(), (kind, key)
        assert h.stats()["view_points"] == 2 * n and fresh.stats()["view_points"] == 0
    finally:
        h.close()
        fresh.close()


# ---- 5. prefetch --------------------------------------------------------------------------------------------------------------

def test_prefetch(handle):
    from chronoclust_amd.scaling.scaler import Scaler
    n, d = 300, 13
    x = values(np.float32, n, d, turn=1)
    wide = widened(x)
    sc = Scaler()
    sc.fit_scaler(wide)
    for scaling in (None, (sc.scale_, sc.min_)):
        exp = referee(handle, wide, scaling)
        upload = handle.points_upload if scaling is None else (lambda v: handle.points_upload_scaled(v, *scaling))
        pre = handle.points_prefetch if scaling is None else (lambda v: handle.points_prefetch(v, *scaling))
        for name in ("Fortran pitched", "C pitched", "Fortran dense", "C wide pitch"):
            a = LAYOUTS[name](x)
            before = handle.stats()["view_points"]
            pre(a)
            upload(a)  # adopted
            assert handle.stats()["view_points"] == before + n
            got = resident(handle, d)
            same_bits(got[0], exp[0], "prefetched %s row-major" % name)
            same_bits(got[1], exp[1], "prefetched %s dimension-major" % name)
            pre(a)
            upload(wide)  # the dense float64 array: discarded
            got = resident(handle, d)
            same_bits(got[0], exp[0], "a float64 array behind a prefetched view")
    # one address, other descriptors: a prefetch of the one is not the upload of the other
    buf = np.zeros(64 * 64, dtype=np.float32)
    buf[:] = np.random.default_rng(2).uniform(0.5, 1.5, buf.size).astype(np.float32)
    as_cols = buf.reshape(64, 64).T                      # float32, columns form, 64 x 64
    as_rows = buf.reshape(64, 64)[:, :63]                # float32, rows form at the same address, 64 x 63
    as_cols63 = buf[:64 * 63].reshape(63, 64).T          # columns form, 64 x 63: shape of as_rows, other strides
    as_u16 = buf.view(np.uint16)[:64 * 126].reshape(126, 64).T[:, :63]  # uint16 at the same address, shape and strides of as_cols63
    assert len({v.ctypes.data for v in (as_cols, as_rows, as_cols63, as_u16)}) == 1
    assert as_u16.shape == as_cols63.shape and [s // 2 for s in as_u16.strides] == [s // 4 for s in as_cols63.strides]
    for first, second in ((as_rows, as_cols63), (as_cols63, as_rows), (as_cols63, as_u16), (as_u16, as_cols63), (as_cols, as_cols63)):
        handle.points_prefetch(first)
        handle.points_upload(second)
        same_bits(handle.points_download(second.shape[1]), widened(second), "another view of a prefetched address")
    # scaled prefetch, plain upload of the same view, and other scaling: not this upload
    a = f_pitched(x)
    handle.points_prefetch(a, sc.scale_, sc.min_)
    handle.points_upload(a)
    same_bits(handle.points_download(d), wide, "plain upload behind a scaled prefetch")
    handle.points_prefetch(a, sc.scale_, sc.min_)
    handle.points_upload_scaled(a, sc.scale_ * 0.5, sc.min_)
    same_bits(handle.points_download(d), wide * (sc.scale_ * 0.5) + sc.min_, "other scaling behind a scaled prefetch")


# ---- 6. the online phase end to end ---------------------------------------------------------------------------------------------

# width -> (points, blobs, tuning): 5 and 20 the ladder, 13 padded operands, 80 the sequential band (k_seq_g)
WIDTHS = {5: (2000, 30, dict(sequential=1)), 13: (2000, 40, dict(sequential=1)), 20: (4000, 200, dict(sequential=1)), 80: (2000, 15, {})}
_streams = {}


def stream(d):
    if d not in _streams:
        n, g, _ = WIDTHS[d]
        over = dict(param_epsilon=0.08) if d >= 80 else {}
        cfg = scenarios.params_to_config(scenarios.blob_params(n, **over))
        _streams[d] = (cfg, [scenarios.make_blobs(9000 + 10 * d + t, n, d, g, 0.01) for t in range(2)])
    return _streams[d]


def run_stream(cfg, Xs, tuning, scaling=None, hdd=None):
    from chronoclust_amd.clustering.hddstream import HDDStream
    h = hdd if hdd is not None else HDDStream(cfg, tuning=tuning or None)
    out = []
    for t, X in enumerate(Xs):
        h.online_microcluster_maintenance(X, t, device_scaling=scaling)
        out.append(dict(uid=h.labels_uid.copy(), path=h.labels_path.copy(), tables=[h.table(k) for k in (0, 1)],
                        counters=(h.pcore_MC_last_id, h.outlier_MC_last_id),
                        members=[list(c.members_in_merge_order) for c in h.final_clusters], stats=h.stats(),
                        resident=h.resident_points(), points_of=h._points_of(int(h.labels_uid[0]))))
    return h, out


def same_run(a, b, what, counted):
    assert len(a) == len(b)
    for t, (ra, rb) in enumerate(zip(a, b)):
        for key in ("uid", "path"):
            diff = T._first_diff(ra[key], rb[key])
            assert diff is None, "%s t=%d %s per point: %s" % (what, t, key, diff)
        for kind in (0, 1):
            for key in T.KEYS:
                assert ra["tables"][kind][key].tobytes() == rb["tables"][kind][key].tobytes(), (what, t, kind, key)
        assert ra["counters"] == rb["counters"] and ra["members"] == rb["members"], (what, t)
        same_bits(ra["resident"], rb["resident"], "%s t=%d resident points" % (what, t))
        assert ra["points_of"] == rb["points_of"], (what, t)
        for key, val in rb["stats"].items():
            if key not in TIME_FIELDS and key != "view_points":
                assert ra["stats"][key] == val, "%s t=%d cc_stats.%s: %r / %r" % (what, t, key, ra["stats"][key], val)
        assert ra["stats"]["view_points"] == counted[t] and rb["stats"]["view_points"] == 0, (what, t)


@pytest.mark.parametrize("d,prune", [(5, None), (13, None), (20, None), (80, None), (20, 2)],
                         ids=["d5", "d13", "d20", "d80", "d20-pruned_forced"])
def test_the_online_phase_does_not_notice(d, prune):
    cfg, Xs = stream(d)
    tuning = WIDTHS[d][2]
    counted = np.cumsum([len(x) for x in Xs]).tolist()
    quantised = [np.rint(x * 50000.0).astype(np.uint16) for x in Xs]
    unscale = (np.full(d, 1.0 / 50000.0), np.zeros(d))
    feeds = [("Fortran float64", [np.asfortranarray(x) for x in Xs], None),
             ("C pitched float32", [c_pitched(x.astype(np.float32)) for x in Xs], None),
             ("uint16", quantised, unscale),
             ("Fortran pitched uint16", [f_pitched(q) for q in quantised], unscale)]
    with knobs(**({} if prune is None else dict(CHRONOCLUST_HIP_PRUNE=prune))):
        for what, arrays, scaling in feeds:
            assert all(not a.flags["C_CONTIGUOUS"] or a.dtype == np.uint16 for a in arrays)
            h_exp, exp = run_stream(cfg, [widened(a) for a in arrays], tuning, scaling)
            h_got, got = run_stream(cfg, arrays, tuning, scaling)
            same_run(got, exp, "d=%d %s" % (d, what), counted)
            if scaling is None:
                assert h_got._X is not None and h_got._X.dtype == np.float64  # (kept as it came, widened on demand by _points_of)
            if prune == 2:
                assert sum(r["stats"]["scan_p_launches"] for r in got) > 0  # (x_absmax was read by a pruned scan)
    if d == 20 and prune is None:  # two equal wrong answers must not pass: the CPU restatement on the same values
        from oracle import oracle as O
        o = O.OracleHDDStream(cfg)
        _, got = run_stream(cfg, feeds[0][1], tuning)
        for t, x in enumerate(Xs):
            o.online_microcluster_maintenance(x, t)
            assert np.array_equal(got[t]["uid"], o.labels_uid) and np.array_equal(got[t]["path"], o.paths)
            assert got[t]["members"] == [[int(v) for v in c["members"]] for c in o.clusters]


# ---- 7. cc_assign through views ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [64, 100])
def test_assign_through_views(chunk):
    from chronoclust_amd import _lib
    cfg, Xs = stream(13)
    with knobs(CHRONOCLUST_HIP_ASSIGN_CHUNK=chunk, CHRONOCLUST_HIP_INGEST_SLAB=128):
        hdd, _ = run_stream(cfg, Xs[:1], WIDTHS[13][2])
    h = hdd._h

    def snapshot():
        return ([{k: v.tobytes() for k, v in h.export(kind).items()} for kind in (_lib.PCORE, _lib.OUTLIER)], h.counters(),
                tuple(a.tobytes() for a in h.labels_download()))

    before = snapshot()
    q64 = np.vstack([Xs[0][500:600], Xs[1][:65]])  # points of the clustered timepoint and strangers: more than one path
    q32 = q64.astype(np.float32)
    for what, query in (("Fortran float64", np.asfortranarray(q64)), ("C pitched float32", c_pitched(q32)),
                        ("Fortran pitched float32", f_pitched(q32)), ("C wide pitch float32", LAYOUTS["C wide pitch"](q32))):
        assert _lib.points_source(query)[1] is not None
        exp = h.assign(widened(query), want_dist=True)
        launches = h.stats()["assign_launches"]
        counted = h.stats()["view_points"]
        got = h.assign(query, want_dist=True)
        A.same_assign(got, exp, "%s chunk=%d" % (what, chunk))
        same_bits(got[2], exp[2], "%s chunk=%d dist" % (what, chunk))
        assert h.stats()["assign_launches"] == launches == -(-165 // chunk)
        assert h.stats()["assign_points"] == 165 and h.stats()["view_points"] == counted + 165
        assert len(set(got[1].tolist())) > 1, "the queries all took one path: nothing was compared"
    assert snapshot() == before, "an assign moved the table or the labels"


def test_assign_takes_a_default_chunk_of_a_pitched_view_in_sub_slabs():
    """The library's own chunk (262 144 points at d = 13) and a float64 view at a pitch of 8 d: 50 000 points are one chunk
    of 41.6 MB of pitched rows, which crosses the set's 16 MiB of staging in three sub-slabs (20 160 points each, the last
    partial); a Fortran-order float32 query of the same points in one."""
    from chronoclust_amd import _lib
    cfg, Xs = stream(13)
    hdd, _ = run_stream(cfg, Xs[:1], WIDTHS[13][2])
    h = hdd._h
    n, d = 50000, 13
    q64 = np.vstack([Xs[0], Xs[1]] * 13)[:n]
    exp = h.assign(q64, want_dist=True)
    assert h.stats()["assign_launches"] == 1
    pitched = c_pitched(q64, extra=7 * d, first=3)
    assert pitched.strides == (8 * d * 8, 8) and _lib.points_source(pitched)[1] is not None
    for what, query in (("float64 at a pitch of 8 d", pitched), ("Fortran float32", np.asfortranarray(q64.astype(np.float32)))):
        want = exp if query.dtype == np.float64 else h.assign(widened(query), want_dist=True)
        got = h.assign(query, want_dist=True)
        A.same_assign(got, want, what)
        same_bits(got[2], want[2], what + " dist")
        assert h.stats()["assign_launches"] == 1 and h.stats()["assign_points"] == n
    pitched[45000, 5] = np.inf  # in the last sub-slab
    with pytest.raises(ValueError, match="non-finite"):
        h.assign(pitched)


# ---- 8. the scaler and app.run -------------------------------------------------------------------------------------------------

def test_col_minmax_of_views(handle):
    from chronoclust_amd.scaling.scaler import Scaler
    for n, d in [(1, 3), (300, 1), (300, 7), (1000, 20), (700, 257), (520, 1024)]:
        x = values(np.float64, n, d, turn=d)
        if n > 1:
            rng = np.random.default_rng(n + d)
            x[rng.integers(0, n, max(1, n // 10)), rng.integers(0, d, max(1, n // 10))] = np.nan
            x[:, d // 2] = np.abs(x[:, d // 2])
            x[n // 3, d // 2], x[n // 2, d // 2], x[n // 4, d // 2] = 0.0, -0.0, np.nan  # NaN, +0.0 and -0.0 in one column
        exp = handle.col_minmax(widened(x))
        for a in [np.asfortranarray(x), f_pitched(x), c_pitched(x)] + ([LAYOUTS["C wide pitch"](x)] if d <= 20 else []):
            if a.flags["C_CONTIGUOUS"]:
                continue
            got = handle.col_minmax(a)
            for g, e, which in zip(got, exp, ("minima", "maxima")):
                assert np.array_equal(g, e), "%s of %d x %d: %r / %r" % (which, n, d, g, e)  # (== : the sign of a zero is free)
            fits = []
            for lo, hi in (got, exp):
                sc = Scaler()
                sc._finish_fit(lo.copy(), hi.copy())
                fits.append(sc)
            same_bits(fits[0].scale_, fits[1].scale_, "scale_ of %d x %d" % (n, d))
            same_bits(fits[0].min_, fits[1].min_, "min_ of %d x %d" % (n, d))
    for dtype in NARROW:
        x = values(dtype, 300, 9)
        exp = handle.col_minmax(widened(x))
        for a in (x, f_pitched(x), c_pitched(x)):
            got = handle.col_minmax(a)
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), np.dtype(dtype).name


def test_app_run_on_csv_files_takes_them_as_parsed(tmp_path, monkeypatch):
    """Three small CSV timepoints: result.csv and every cluster_points_D{t}.csv byte for byte those of a run whose CSVs were
    first converted to C-contiguous float64 `.npy`; the CSV run hands the HDDStream the parsed, column-major array."""
    import pandas as pd
    from chronoclust_amd import app
    from golden_util import GOLDEN
    from test_app_end_to_end import _reset_logging
    c1 = os.path.join(GOLDEN, "c1")
    seen, made = [], []

    class Recording(app.HDDStream):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

        def online_microcluster_maintenance(self, input_dataset, *a, **kw):
            seen.append(input_dataset)
            return super().online_microcluster_maintenance(input_dataset, *a, **kw)

    monkeypatch.setattr(app, "HDDStream", Recording)
    csvs, npys, total = [], [], 0
    for t in range(3):
        frame = pd.read_csv(os.path.join(c1, "synthetic_d%d.csv.gz" % t)).iloc[:1500]
        fn = os.path.join(str(tmp_path), "tp%d.csv" % t)
        frame.to_csv(fn, index=False)
        csvs.append(fn)
        parsed = pd.read_csv(fn).to_numpy()
        assert not parsed.flags["C_CONTIGUOUS"]
        np.save(fn[:-4] + ".npy", np.ascontiguousarray(parsed, dtype=np.float64))
        npys.append(fn[:-4] + ".npy")
        with open(fn[:-4] + ".npy.columns", "w") as f:  # (the CSV's header: app.run names the output columns by it)
            f.write("\n".join(frame.columns) + "\n")
        total += len(parsed)
    outs = []
    for files in (csvs, npys):
        out = os.path.join(str(tmp_path), "out_" + files[0][-3:])
        os.makedirs(out)
        try:
            app.run(data=files, output_directory=out, **scenarios.C1_PARAMS)
        finally:
            _reset_logging()
        outs.append(out)
    for fn in ["result.csv"] + ["cluster_points_D%d.csv" % t for t in range(3)]:
        a, b = (open(os.path.join(o, fn), "rb").read() for o in outs)
        assert a == b and len(a) > 0, fn
    assert len(seen) == 6
    assert all(isinstance(x, np.ndarray) and x.flags["F_CONTIGUOUS"] and not x.flags["C_CONTIGUOUS"] for x in seen[:3])
    assert all(x.flags["C_CONTIGUOUS"] for x in seen[3:])
    assert [m.stats()["view_points"] for m in made] == [total, 0] and total > 0


# ---- 9. a group -------------------------------------------------------------------------------------------------------------------

def test_a_group_of_two_fed_a_column_major_array():
    from chronoclust_amd import _lib
    name = "stale-3000+1096x20"
    pcores, outliers, par, X, meta = T.build_online(name)
    xf = np.asfortranarray(X)
    assert _lib.points_source(xf)[1] is not None
    h = _lib.Handle(0)
    try:
        single = T.handle_online(h, (pcores, outliers, par, widened(X), meta))
        lists = [h.export(kind) for kind in (0, 1)]
        counters = h.counters()
    finally:
        h.close()
    dense_hs, _, dense_stats = T.group_online(2, (pcores, outliers, par, widened(X), meta))
    for g in dense_hs:
        g.close()
    hs, labels, stats = T.group_online(2, (pcores, outliers, par, xf, meta))
    try:
        for rank in range(2):
            for key, a, b in (("uid", labels[rank][0][0], single[0][0]), ("path", labels[rank][0][1], single[0][1])):
                diff = T._first_diff(a, b)
                assert diff is None, "rank %d %s: %s" % (rank, key, diff)
            for kind in (0, 1):
                got = hs[rank].export(kind)
                for key in T.KEYS:
                    assert got[key].tobytes() == lists[kind][key].tobytes(), (rank, kind, key)
            assert hs[rank].counters() == counters
            assert stats[rank]["view_points"] == len(xf) and dense_stats[rank]["view_points"] == 0  # counted per rank
            assert stats[rank]["comm_launches"] == dense_stats[rank]["comm_launches"], (stats[rank], dense_stats[rank])
            assert stats[rank]["sharded_windows"] > 0, stats[rank]
    finally:
        for g in hs:
            g.close()
