"""List-mode event records end to end (cc_points_upload_list and its kin, k_ingest_list): what the device holds after the
bytes of an FCS DATA segment went in as they lie - either byte order, the clustered channels a list of the record's columns,
integer channels under their range masks - is, bit for bit, what it holds after the same values were decoded on the host and
went in as C-contiguous float64: the row-major copy, the dimension-major copy with its pad rows, the flag words; so labels,
tables, clusters and every counter of the online phase, the answers of the read-only assignment and the scaler's fit are the
same.  The expectation is always the float64 route fed np.ascontiguousarray(np.asarray(list_mode, np.float64)); every
comparison is of bit patterns, nothing is tolerated.  The record buffers are written by fcs_util (bytes moved plane by plane,
no byte-order conversion of numpy's) and the host decode itself is checked against the native array they were written from.
Shapes: the smallest that cross a point tile (64), a block of dimensions (64), a padded scan width, a slab
(CHRONOCLUST_HIP_INGEST_SLAB=128: 300 events are three slabs, the last partial) and a chunk of cc_assign."""
import ctypes

import numpy as np
import pytest

import assign_util as A
import fcs_util as F
import scenarios
import table_util as T
from pipeline_util import knobs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

NS = (1, 63, 64, 65, 129, 300)
DS = (1, 3, 9, 20, 64, 65, 130)
SLABS = (None, 128)
DTYPES = (np.float32, np.float64, np.uint8, np.uint16, np.uint32)
LITTLE, BIG = (1, 2, 3, 4), (4, 3, 2, 1)
COLUMN_LISTS = ("identity", "reversed", "shuffle with one repeat", "every other channel")
TIME_FIELDS = ("scan_ms", "run_ms", "comm_ms", "scan_ms_pruned", "calib_allgather_us", "calib_scan_ns_per_row_dim")
MASKS = (0xFFFFFFFF, 0x3FF, 0x0F, 0x7FFF, 0x1, 0xFFFFF)


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float64
    return a.view(np.int64)


def same_bits(got, exp, what):
    diff = None if np.array_equal(bits(got), bits(exp)) else T._first_diff(bits(got), bits(exp))
    assert diff is None, "%s: %s" % (what, diff)


def widened(lm):
    """What the float64 route is fed: the referee's input."""
    return np.ascontiguousarray(np.asarray(lm, dtype=np.float64))


def src_cols_of(d):
    return (d, d + 3, 8 * d + 1)


def column_list(kind, d, src_cols, rng):
    if kind == "identity":
        return np.arange(d)
    if kind == "reversed":
        return np.arange(src_cols - 1, src_cols - 1 - d, -1)
    if kind == "shuffle with one repeat":
        cols = rng.permutation(src_cols)[:d]
        if d > 1:
            cols[-1] = cols[0]
        return cols
    return (2 * np.arange(d)) % src_cols  # (every other channel; around the record's end where it is short)


def specials(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        f = np.finfo(dtype)
        return np.array([0.0, -0.0, f.smallest_subnormal, -f.smallest_subnormal, np.nextafter(f.tiny, dtype.type(0)), f.tiny,
                         f.max, -f.max], dtype=dtype)
    i = np.iinfo(dtype)
    return np.array([0, 1, i.max, i.max - 1, i.max // 2 + 1], dtype=dtype)  # (UINT32_MAX among them)


def records(dtype, n, src_cols, cols, turn=0, fill_unselected=True):
    """Native [n, src_cols] of the type: random values, a special value at element 0 of the selection, at its last element and
    at the end of the first point tile - which one: by `turn` - and all of them scattered; the floating types hold NaN
    patterns (quiet and signalling, both signs) in every channel the selection does not name."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(1000 * n + src_cols + dtype.itemsize)
    if dtype.kind == "f":
        rec = rng.uniform(-4.0, 4.0, (n, src_cols)).astype(dtype)
    else:
        rec = rng.integers(0, np.iinfo(dtype).max, (n, src_cols), dtype=dtype, endpoint=True)
    sp = specials(dtype)
    if n * len(cols) > 40:
        for k in range(2 * len(sp)):
            rec[rng.integers(0, n), cols[rng.integers(0, len(cols))]] = sp[k % len(sp)]
    for k, (r, c) in enumerate(((0, cols[0]), (n - 1, cols[-1]), (min(n, 64) - 1, cols[-1]))):
        rec[r, c] = sp[(turn + k) % len(sp)]
    if dtype.kind == "f" and fill_unselected:
        nan_bits = {4: (0x7FC00000, 0xFFC00001, 0x7F800001, 0xFF800001, 0x7F800000), 8: (0x7FF8000000000000, 0xFFF8000000000001,
                    0x7FF0000000000001, 0xFFF0000000000001, 0x7FF0000000000000)}[dtype.itemsize]
        image = rec.view("u%d" % dtype.itemsize)
        for j, c in enumerate(sorted(set(range(src_cols)) - set(int(v) for v in cols))):
            image[:, c] = nan_bits[j % len(nan_bits)]  # (NaN patterns and +Inf: never read)
    return rec


def list_mode(rec, order, cols=None, masks=None):
    """The ListMode of native records `rec`, written in byte order `order`, one byte past an aligned address."""
    from chronoclust_amd import _lib
    buf = F.unaligned(F.fast_records(rec, order))
    dt = rec.dtype.newbyteorder("<" if order == LITTLE else ">") if rec.dtype.itemsize > 1 else rec.dtype
    lm = _lib.ListMode(buf, rec.shape[0], rec.shape[1], dt, columns=cols, masks=masks)
    assert lm._bytes.ctypes.data % 64 == 1 or rec.size == 0
    return lm


def native_decode(rec, cols, masks):
    """What the selection holds, from the native array the records were written from: the check on ListMode's own decode."""
    out = rec[:, cols]
    if masks is not None:
        out = out & np.asarray(masks, np.uint32).astype(rec.dtype)
    return np.ascontiguousarray(out.astype(np.float64))


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
    """The float64 route on the host-decoded dense array: (row-major copy, dimension-major copy)."""
    from chronoclust_amd import _lib
    n, d = wide.shape
    before = h.stats()
    if scaling is None:
        h.points_upload(wide)
    else:
        h.points_upload_scaled(wide, *scaling)
    after = h.stats()
    assert all(after[k] == before[k] for k in ("list_points", "view_points", "f32_points"))
    x, xt = resident(h, d)
    assert xt.shape == (_lib.xt_rows(d), n) and not bits(xt[d:]).any()
    same_bits(xt[:d], x.T, "the referee's own two copies")
    return x, xt


def check_list(h, lm, exp, what, scaling=None):
    """`lm` goes in as it lies; the two resident copies are the referee's, and the counters say which route it took."""
    n, d = lm.shape
    before = h.stats()
    if scaling is None:
        h.points_upload(lm)
    else:
        h.points_upload_scaled(lm, *scaling)
    after = h.stats()
    assert after["list_points"] == before["list_points"] + n, what
    assert after["view_points"] == before["view_points"] and after["f32_points"] == before["f32_points"], what
    x, xt = resident(h, d)
    same_bits(x, exp[0], what + " row-major")
    assert xt.shape == exp[1].shape, what
    same_bits(xt, exp[1], what + " dimension-major with its pad rows")


# ---- 1. ingest alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
def test_ingest_alone(handle, n):
    """Every dtype, swapped and native, every d, every src_cols; the four column lists turn with (dtype, order, d, src_cols)
    so that every list meets every dtype, either order and every src_cols form within one n."""
    seen = set()
    turn = NS.index(n)
    for ti, dtype in enumerate(DTYPES):
        for oi, order in enumerate((LITTLE, BIG)):
            for di, d in enumerate(DS):
                for si, src_cols in enumerate(src_cols_of(d)):
                    kind = COLUMN_LISTS[(turn + ti + oi + di + si) % 4]
                    rng = np.random.default_rng(n + 7 * d + src_cols)
                    cols = column_list(kind, d, src_cols, rng)
                    rec = records(dtype, n, src_cols, cols, turn=turn + di)
                    masks = None
                    if np.dtype(dtype).kind == "u" and (di + si) % 2:
                        masks = [0x0F] + [MASKS[(c + di) % len(MASKS)] for c in range(1, d)]  # (the first one bites in every type)
                    lm = list_mode(rec, order, cols, masks)
                    wide = widened(lm)
                    same_bits(wide, native_decode(rec, cols, masks), "ListMode's decode against the native array")
                    if masks is not None and n * d > 20:
                        assert (wide != rec[:, cols].astype(np.float64)).any(), "no stored value had a bit above its mask"
                    exp = referee(handle, wide)
                    same_bits(exp[0], wide, "the referee holds the decoded values")
                    check_list(handle, lm, exp, "%s %s %d x %d of %d, %s%s" % (np.dtype(dtype).name, "big" if order == BIG else "little",
                                                                                 n, d, src_cols, kind, ", masked" if masks else ""))
                    seen.add((ti, kind))
                    seen.add((oi + 10, kind))
                    seen.add((si + 20, kind))
    assert len(seen) == 4 * (len(DTYPES) + 2 + 3)


def test_default_columns_and_masks_at_the_c_level(handle):
    """cols NULL is 0 .. d - 1 of a wider record, masks NULL is none; UINT32_MAX survives, big-endian."""
    from chronoclust_amd import _lib
    rec = records(np.uint32, 70, 9, np.arange(5))
    rec[0, 0], rec[69, 4] = 0xFFFFFFFF, 0xFFFFFFFE
    lm = list_mode(rec, BIG, np.arange(5))
    desc = lm.descriptor()
    desc.cols = None
    exp = referee(handle, native_decode(rec, np.arange(5), None))
    handle._check(handle._lib.cc_points_upload_list(handle._h, ctypes.byref(desc), None, None))
    handle._n = 70
    x, xt = resident(handle, 5)
    same_bits(x, exp[0], "cols NULL")
    same_bits(xt, exp[1], "cols NULL, dimension-major")
    assert x[0, 0] == 4294967295.0


# ---- 2. NaN / Inf --------------------------------------------------------------------------------------------------------------

def test_non_finite_in_a_selected_channel_is_refused_and_elsewhere_is_not():
    from chronoclust_amd import _lib
    n, src_cols = 300, 9
    cols = np.array([7, 2, 4, 2, 5])  # (five dimensions: the table's)
    with knobs(CHRONOCLUST_HIP_INGEST_SLAB=128, CHRONOCLUST_HIP_ASSIGN_CHUNK=128):
        h = _lib.Handle(0)
    try:
        pcores, outliers, par, X = A.case("stale-31+33x5")[:4]
        T.fill_handle(h, par, pcores, outliers)
        for dtype in (np.float32, np.float64):
            for order in (LITTLE, BIG):
                clean = records(dtype, n, src_cols, cols)
                clean = np.clip(clean, -4.0, 4.0)  # (the unselected channels hold NaN patterns and Inf: clip keeps NaN)
                assert np.isnan(clean[:, 0]).all() and np.isfinite(clean[:, cols]).all()
                lm = list_mode(clean, order, cols)
                exp = referee(h, widened(lm))
                check_list(h, lm, exp, "NaN patterns in unselected channels only")
                for value in (np.nan, np.inf, -np.inf):
                    for r, c in ((0, 7), (n - 1, 2), (270, 4), (200, 2)):
                        bad = clean.copy()
                        bad[r, c] = value
                        lm = list_mode(bad, order, cols)
                        with pytest.raises(ValueError, match="non-finite"):
                            h.points_upload(lm)
                        h.points_prefetch(lm)
                        with pytest.raises(ValueError, match="non-finite"):
                            h.points_upload(lm)
                # a signalling NaN pattern in a selected channel, written as bytes
                bad = clean.copy()
                bad.view("u%d" % bad.dtype.itemsize)[150, 4] = 0x7F800001 if bad.dtype.itemsize == 4 else 0x7FF0000000000001
                with pytest.raises(ValueError, match="non-finite"):
                    h.points_upload(list_mode(bad, order, cols))
        d5 = np.arange(5)
        clean5 = np.clip(records(np.float32, n, 8, d5), -4.0, 4.0)
        bad5 = clean5.copy()
        bad5[290, 3] = np.inf
        with pytest.raises(ValueError, match="non-finite"):
            h.assign(list_mode(bad5, BIG, d5))
        uid = h.assign(list_mode(clean5, BIG, d5))[0]
        assert uid.shape == (n,)
    finally:
        h.close()


# ---- 3. scaled upload, col_minmax, the scaler's fit ------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d", [(1, 3), (65, 13), (129, 20), (300, 9), (129, 130)])
def test_scaled(handle, n, d):
    from chronoclust_amd.scaling.scaler import Scaler
    for i, dtype in enumerate(DTYPES):
        src_cols = src_cols_of(d)[i % 3]
        cols = column_list(COLUMN_LISTS[(i + n) % 4], d, src_cols, np.random.default_rng(d))
        rec = records(dtype, n, src_cols, cols, turn=n + d)
        if np.dtype(dtype).kind == "f":
            image = rec.view("u%d" % rec.dtype.itemsize).copy()
            rec = np.clip(rec, -1e30, 1e30)  # (a range whose reciprocal is a normal number)
            sel = np.zeros(src_cols, bool)
            sel[cols] = True
            rec.view(image.dtype)[:, ~sel] = image[:, ~sel]
        masks = [MASKS[c % len(MASKS)] for c in range(d)] if np.dtype(dtype).kind == "u" else None
        for order in (LITTLE, BIG):
            lm = list_mode(rec, order, cols, masks)
            wide = widened(lm)
            sc = Scaler()
            sc.fit_scaler(wide)
            scaling = (sc.scale_, sc.min_)
            exp = referee(handle, wide, scaling)
            same_bits(exp[0], wide * sc.scale_ + sc.min_, "the referee holds numpy's two roundings")
            check_list(handle, lm, exp, "scaled %s %d x %d of %d" % (np.dtype(dtype).name, n, d, src_cols), scaling=scaling)


def test_a_scale_that_overflows_is_refused_as_on_the_float64_route(handle):
    for dtype in (np.float32, np.uint16):
        cols = np.array([4, 1, 6, 0, 2])
        rec = records(dtype, 300, 8, cols)
        if dtype == np.float32:
            rec[200, 0] = 1e30
        lm = list_mode(rec, BIG, cols)
        scale, min_ = np.ones(5), np.zeros(5)
        for a in (widened(lm), lm):
            handle.points_upload_scaled(a, scale, min_)
        scale[3] = 1e305
        for a in (widened(lm), lm):
            with pytest.raises(ValueError, match="non-finite"):
                handle.points_upload_scaled(a, scale, min_)


def test_col_minmax_and_the_scalers_fit(handle):
    from chronoclust_amd.scaling.scaler import Scaler
    for i, (n, d) in enumerate([(1, 3), (300, 1), (300, 7), (1000, 20), (700, 257), (300, 130)]):
        for j, dtype in enumerate(DTYPES):
            src_cols = src_cols_of(d)[(i + j) % 3] if d < 200 else d + 3
            cols = column_list(COLUMN_LISTS[(i + j) % 4], d, src_cols, np.random.default_rng(i))
            rec = records(dtype, n, src_cols, cols, turn=j)
            if np.dtype(dtype).kind == "f":
                rec[:, cols] = np.clip(rec[:, cols], -1e30, 1e30)  # (a range that float64 holds)
            if np.dtype(dtype).kind == "f" and n > 1:
                rng = np.random.default_rng(n + d)
                rec[rng.integers(0, n, max(1, n // 10)), cols[rng.integers(0, d, max(1, n // 10))]] = np.nan  # (ignored)
                c = cols[d // 2]
                rec[:, c] = np.abs(rec[:, c])
                rec[n // 3, c], rec[n // 2, c], rec[n // 4, c] = 0.0, -0.0, np.nan
            masks = [MASKS[(c + 1) % len(MASKS)] for c in range(d)] if np.dtype(dtype).kind == "u" and i % 2 else None
            lm = list_mode(rec, (LITTLE, BIG)[(i + j) % 2], cols, masks)
            wide = widened(lm)
            exp = handle.col_minmax(wide)
            before = handle.stats()["list_points"]
            got = handle.col_minmax(lm)
            assert handle.stats()["list_points"] == before  # (a reduction takes no points in)
            for g, e, which in zip(got, exp, ("minima", "maxima")):
                assert np.array_equal(g, e), "%s of %s %d x %d: %r / %r" % (which, np.dtype(dtype).name, n, d, g, e)  # (== : the sign of a zero is free)
            fits = []
            for lo, hi in (got, exp):
                sc = Scaler()
                sc._finish_fit(lo.copy(), hi.copy())
                fits.append(sc)
            same_bits(fits[0].scale_, fits[1].scale_, "scale_ of %d x %d" % (n, d))
            same_bits(fits[0].min_, fits[1].min_, "min_ of %d x %d" % (n, d))


# ---- 4. prefetch ---------------------------------------------------------------------------------------------------------------

def test_prefetch(handle):
    from chronoclust_amd import _lib
    from chronoclust_amd.scaling.scaler import Scaler
    n, d, src_cols = 300, 13, 16
    cols = column_list("shuffle with one repeat", d, src_cols, np.random.default_rng(4))
    masks = [MASKS[c % len(MASKS)] for c in range(d)]
    rec = records(np.uint16, n, src_cols, cols, turn=1)
    lm = list_mode(rec, BIG, cols, masks)
    wide = widened(lm)
    sc = Scaler()
    sc.fit_scaler(wide)
    for scaling in (None, (sc.scale_, sc.min_)):
        exp = referee(handle, wide, scaling)
        upload = handle.points_upload if scaling is None else (lambda v: handle.points_upload_scaled(v, *scaling))
        pre = handle.points_prefetch if scaling is None else (lambda v: handle.points_prefetch(v, *scaling))
        before = handle.stats()["list_points"]
        pre(lm)
        upload(lm)  # adopted
        assert handle.stats()["list_points"] == before + n
        got = resident(handle, d)
        same_bits(got[0], exp[0], "prefetched row-major")
        same_bits(got[1], exp[1], "prefetched dimension-major")
        # the same bytes behind an equal descriptor built anew: adopted too (nothing to tell apart)
        pre(lm)
        upload(_lib.ListMode(lm.buffer, n, src_cols, lm.dtype, columns=cols.copy(), masks=list(masks)))
        same_bits(resident(handle, d)[0], exp[0], "an equal descriptor")
        pre(lm)
        upload(wide)  # the dense float64 array: discarded
        same_bits(resident(handle, d)[0], exp[0], "a float64 array behind prefetched records")
    # one address; only the column list, only the masks, only the flag differ: a prefetch of the one is not the upload of the other
    other_cols = cols.copy()
    other_cols[3] = (other_cols[3] + 1) % src_cols
    other_masks = list(masks)
    other_masks[5] ^= 0x4
    variants = {"the column list": _lib.ListMode(lm.buffer, n, src_cols, lm.dtype, columns=other_cols, masks=masks),
                "the masks": _lib.ListMode(lm.buffer, n, src_cols, lm.dtype, columns=cols, masks=other_masks),
                "no masks": _lib.ListMode(lm.buffer, n, src_cols, lm.dtype, columns=cols),
                "the flag": _lib.ListMode(lm.buffer, n, src_cols, lm.dtype.newbyteorder(), columns=cols, masks=masks)}
    for what, other in variants.items():
        assert other._bytes.ctypes.data == lm._bytes.ctypes.data
        want = widened(other)
        assert not np.array_equal(want, wide), what
        for first, second, exp_values in ((lm, other, want), (other, lm, wide)):
            handle.points_prefetch(first)
            handle.points_upload(second)
            same_bits(handle.points_download(d), exp_values, "only %s differ" % what)
    # scaled prefetch, plain upload of the same records, and other scaling: not this upload
    handle.points_prefetch(lm, sc.scale_, sc.min_)
    handle.points_upload(lm)
    same_bits(handle.points_download(d), wide, "plain upload behind a scaled prefetch")
    handle.points_prefetch(lm, sc.scale_, sc.min_)
    handle.points_upload_scaled(lm, sc.scale_ * 0.5, sc.min_)
    same_bits(handle.points_download(d), wide * (sc.scale_ * 0.5) + sc.min_, "other scaling behind a scaled prefetch")
    # a prefetch longer than one 16 MiB piece would be; here: more than one slab of 128 where the knob is set
    big = records(np.float32, 1000, 40, np.arange(0, 40, 3))
    lmb = list_mode(big, BIG, np.arange(0, 40, 3))
    exp = referee(handle, widened(lmb))
    handle.points_prefetch(lmb)
    check_list(handle, lmb, exp, "prefetched float32 records, 1000 x 14 of 40")


# ---- 5. the online phase under forced pruning ------------------------------------------------------------------------------------

_streams = {}


def stream(d, n):
    if (d, n) not in _streams:
        g = 40 if d == 13 else 200
        cfg = scenarios.params_to_config(scenarios.blob_params(n))
        _streams[(d, n)] = (cfg, [scenarios.make_blobs(7000 + 10 * d + t + n, n, d, min(g, max(4, n // 20)), 0.01) for t in range(2)])
    return _streams[(d, n)]


def run_stream(cfg, Xs, scaling=None):
    from chronoclust_amd.clustering.hddstream import HDDStream
    h = HDDStream(cfg, tuning=dict(sequential=1))
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
            if key not in TIME_FIELDS and key != "list_points":
                assert ra["stats"][key] == val, "%s t=%d cc_stats.%s: %r / %r" % (what, t, key, ra["stats"][key], val)
        assert ra["stats"]["list_points"] == counted[t] and rb["stats"]["list_points"] == 0, (what, t)


@pytest.mark.parametrize("d,n", [(13, 300), (13, 5000), (20, 300), (20, 5000)])
def test_the_online_phase_under_forced_pruning_does_not_notice(d, n):
    cfg, Xs = stream(d, n)
    counted = np.cumsum([len(x) for x in Xs]).tolist()
    src_cols = d + 5
    cols = column_list("shuffle with one repeat", d, src_cols, np.random.default_rng(d))
    cols[-1] = sorted(set(range(src_cols)) - set(cols.tolist()))[0]  # (no repeat: the blobs' dimensions stay distinct)

    def interleaved(x, dtype):
        rec = np.full((len(x), src_cols), np.nan if np.dtype(dtype).kind == "f" else 9, dtype=dtype)
        rec[:, cols] = x
        return rec

    quantised = [np.rint(x * 50000.0).astype(np.uint16) for x in Xs]
    unscale = (np.full(d, 1.0 / 50000.0), np.zeros(d))
    feeds = [("big-endian float64", [list_mode(interleaved(x, np.float64), BIG, cols) for x in Xs], None),
             ("big-endian float32", [list_mode(interleaved(x.astype(np.float32), np.float32), BIG, cols) for x in Xs], None),
             ("big-endian uint16", [list_mode(interleaved(q, np.uint16), BIG, cols) for q in quantised], unscale)]
    with knobs(CHRONOCLUST_HIP_PRUNE=2):
        for what, lms, scaling in feeds:
            _, exp = run_stream(cfg, [widened(lm) for lm in lms], scaling)
            _, got = run_stream(cfg, lms, scaling)
            same_run(got, exp, "d=%d n=%d %s" % (d, n, what), counted)
            if n >= 5000 and d == 20:
                assert sum(r["stats"]["scan_p_launches"] for r in got) > 0  # (x_absmax was read by a pruned scan)
    same_bits(widened(feeds[0][1][0]), Xs[0], "the float64 records hold the blobs")


# ---- 6. assign, the C level, a group ------------------------------------------------------------------------------------------------

def test_assign_with_a_chunk_of_100():
    from chronoclust_amd import _lib
    cfg, Xs = stream(13, 5000)
    with knobs(CHRONOCLUST_HIP_ASSIGN_CHUNK=100, CHRONOCLUST_HIP_INGEST_SLAB=128):
        hdd, _ = run_stream(cfg, [Xs[0][:2000]])
    h = hdd._h

    def snapshot():
        return ([{k: v.tobytes() for k, v in h.export(kind).items()} for kind in (_lib.PCORE, _lib.OUTLIER)], h.counters(),
                tuple(a.tobytes() for a in h.labels_download()))

    before = snapshot()
    q64 = np.vstack([Xs[0][500:600], Xs[1][:65]])  # points of the clustered timepoint and strangers: more than one path
    cols = np.random.default_rng(1).permutation(20)[:13]
    for what, dtype, order in (("big-endian float64", np.float64, BIG), ("big-endian float32", np.float32, BIG),
                               ("little-endian float32", np.float32, LITTLE)):
        rec = np.full((165, 20), np.nan, dtype=dtype)
        rec[:, cols] = q64.astype(dtype)
        lm = list_mode(rec, order, cols)
        exp = h.assign(widened(lm), want_dist=True)
        launches = h.stats()["assign_launches"]
        counted = h.stats()
        got = h.assign(lm, want_dist=True)
        A.same_assign(got, exp, what)
        same_bits(got[2], exp[2], what + " dist")
        after = h.stats()
        assert after["assign_launches"] == launches == 2 and after["assign_points"] == 165
        assert after["list_points"] == counted["list_points"] + 165
        assert after["view_points"] == counted["view_points"] and after["f32_points"] == counted["f32_points"]
        assert len(set(got[1].tolist())) > 1, "the queries all took one path: nothing was compared"
    assert snapshot() == before, "an assign moved the table or the labels"


def test_online_and_assign_lists_at_the_c_level():
    """cc_online_list and cc_assign_list straight through ctypes (the Python layer uploads, runs and downloads in three calls)."""
    from chronoclust_amd import _lib
    name = "stale-31+33x5"
    pcores, outliers, par, X = A.case(name)[:4]
    n = len(X)
    cols = np.array([6, 0, 3, 7, 2])
    rec = np.full((n, 8), np.nan)
    rec[:, cols] = X
    lm = list_mode(rec, BIG, cols)
    same_bits(widened(lm), X, "the records hold the case's points")
    h, fresh = _lib.Handle(0), _lib.Handle(0)
    try:
        for g in (h, fresh):
            T.fill_handle(g, par, pcores, outliers)
        exp_assign = fresh.assign(np.ascontiguousarray(X), want_dist=True)
        exp = fresh.online(np.ascontiguousarray(X))
        desc = lm.descriptor()
        uid, path, dist = np.empty(n, np.int64), np.empty(n, np.int8), np.empty(n, np.float64)
        h._check(h._lib.cc_assign_list(h._h, ctypes.byref(desc), _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p), _lib._ptr(dist)))
        A.same_assign((uid, path, dist), exp_assign, name + " cc_assign_list")
        uid, path = np.empty(n, np.int64), np.empty(n, np.int8)
        h._check(h._lib.cc_online_list(h._h, ctypes.byref(desc), _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p)))
        assert T._first_diff(uid, exp[0]) is None and T._first_diff(path, exp[1]) is None
        for kind in (0, 1):
            got, want = h.export(kind), fresh.export(kind)
            for key in T.KEYS:
                assert got[key].tobytes() == want[key].tobytes(), (kind, key)
        assert h.stats()["list_points"] == 2 * n and fresh.stats()["list_points"] == 0
        assert h.stats()["view_points"] == 0 and h.stats()["f32_points"] == 0
    finally:
        h.close()
        fresh.close()


def test_a_group_of_two_fed_event_records():
    name = "stale-3000+1096x20"
    pcores, outliers, par, X, meta = T.build_online(name)
    from chronoclust_amd import _lib
    d = X.shape[1]
    cols = np.random.default_rng(2).permutation(d + 4)[:d]
    rec = np.full((len(X), d + 4), np.nan)
    rec[:, cols] = X
    lm = list_mode(rec, BIG, cols)
    wide = widened(lm)
    same_bits(wide, X, "the records hold the case's points")
    h = _lib.Handle(0)
    try:
        single = T.handle_online(h, (pcores, outliers, par, wide, meta))
        lists = [h.export(kind) for kind in (0, 1)]
        counters = h.counters()
    finally:
        h.close()
    dense_hs, _, dense_stats = T.group_online(2, (pcores, outliers, par, wide, meta))
    for g in dense_hs:
        g.close()
    hs, labels, stats = T.group_online(2, (pcores, outliers, par, lm, meta))
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
            assert stats[rank]["list_points"] == len(X) and dense_stats[rank]["list_points"] == 0  # counted per rank
            assert stats[rank]["view_points"] == 0 and stats[rank]["f32_points"] == 0
            assert stats[rank]["comm_launches"] == dense_stats[rank]["comm_launches"], (stats[rank], dense_stats[rank])
            assert stats[rank]["sharded_windows"] > 0, stats[rank]
    finally:
        for g in hs:
            g.close()


# ---- 7. descriptor refusals at the C level ---------------------------------------------------------------------------------------

def test_descriptor_refusals(handle):
    from chronoclust_amd import _lib
    rec = records(np.float32, 40, 8, np.arange(6))
    lm = list_mode(rec, BIG, np.arange(6))
    u16 = list_mode(records(np.uint16, 40, 8, np.arange(6)), BIG, np.arange(6), masks=[0xFF] * 6)
    exp = referee(handle, widened(lm))

    def desc(base=lm, **over):
        out = base.descriptor()
        for k, v in over.items():
            setattr(out, k, v)
        return out

    i32 = ctypes.POINTER(ctypes.c_int32)
    bad_cols = [np.array(v, np.int32) for v in ([0, 1, 8, 2, 3, 4], [0, 1, 2, 3, 4, -1])]
    many = np.zeros(_lib.MAX_DIM + 1, np.int32)
    cases = [("null data", desc(data=None), "null"),
             ("n < 0", desc(n=-1), "n must be"),
             ("d = 0", desc(d=0), "d must be"),
             ("d = 1025", desc(d=_lib.MAX_DIM + 1, cols=many.ctypes.data_as(i32)), "d must be"),
             ("src_cols = 0", desc(src_cols=0), "src_cols"),
             ("src_cols = 4097", desc(src_cols=_lib.MAX_SRC_COLS + 1), "src_cols"),
             ("a column beyond the record", desc(cols=bad_cols[0].ctypes.data_as(i32)), "column 8"),
             ("a negative column", desc(cols=bad_cols[1].ctypes.data_as(i32)), "column -1"),
             ("d > src_cols without a list", desc(cols=None, d=9), "column"),
             ("dtype F16", desc(dtype=_lib.DT_F16), "dtype"),
             ("dtype I32", desc(dtype=_lib.DT_I32), "dtype"),
             ("dtype 99", desc(dtype=99), "dtype"),
             ("unknown flag bits", desc(flags=2), "flag"),
             ("unknown flag bits beside the known one", desc(flags=5), "flag"),
             ("masks with a floating dtype", desc(masks=u16.masks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), "masks"),
             ("an extent beyond int64", desc(n=2 ** 61), "int64")]
    before = handle.stats()
    mn, mx = np.zeros(1025), np.zeros(1025)
    uid, path = np.zeros(40, np.int64), np.zeros(40, np.int8)
    lib, hh = handle._lib, handle._h
    for what, view, reason in cases:
        calls = [lib.cc_points_upload_list(hh, ctypes.byref(view), None, None),
                 lib.cc_points_prefetch_list(hh, ctypes.byref(view), None, None),
                 lib.cc_col_minmax_list(hh, ctypes.byref(view), _lib._ptr(mn), _lib._ptr(mx)),
                 lib.cc_online_list(hh, ctypes.byref(view), _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p)),
                 lib.cc_assign_list(hh, ctypes.byref(view), _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p), None)]
        assert calls == [-2] * 5, (what, calls)  # CC_ERR_BAD_ARG
        assert reason in lib.cc_last_error(hh).decode(), (what, lib.cc_last_error(hh))
        with pytest.raises(ValueError, match="bad argument"):
            handle._check(calls[0])
    # a null descriptor; n = 0 where the sibling needs points; scale without min_
    assert lib.cc_points_upload_list(hh, None, None, None) == -2 and b"null" in lib.cc_last_error(hh)
    assert lib.cc_assign_list(hh, None, _lib._ptr(uid, _lib._i64p), None, None) == -2
    empty = desc(n=0)
    assert lib.cc_points_prefetch_list(hh, ctypes.byref(empty), None, None) == -2 and b"n must be" in lib.cc_last_error(hh)
    assert lib.cc_col_minmax_list(hh, ctypes.byref(empty), _lib._ptr(mn), _lib._ptr(mx)) == -2
    ok = desc()
    assert lib.cc_points_upload_list(hh, ctypes.byref(ok), _lib._ptr(mn), None) == -2
    # nothing moved, nothing was launched or counted: the resident points are the referee's
    after = handle.stats()
    for key in ("list_points", "view_points", "f32_points", "assign_launches", "assign_points", "scan_launches", "scan_u_launches",
                "scan_p_launches", "windows", "points"):
        assert after[key] == before[key], key
    x, xt = resident(handle, 6)
    same_bits(x, exp[0], "resident points behind refused calls")
    same_bits(xt, exp[1], "resident points behind refused calls, dimension-major")
    check_list(handle, lm, exp, "good records behind refused ones")
    # n = 0 is an upload of no points, as on the float64 route
    handle._check(lib.cc_points_upload_list(hh, ctypes.byref(empty), None, None))
    handle._n = 0
    assert handle.points_download(6).shape == (0, 6)
