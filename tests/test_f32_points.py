"""Single-precision points end to end (cc_points_upload_f32 and its kin, k_ingest_f32): what the device holds after a
float32 array went in is, bit for bit, what it holds after the same values were widened on the host and went in as float64 -
the row-major copy, the dimension-major copy with its padded rows, the flag words -, so labels, tables, clusters and every
counter of the online phase, the answers of the read-only assignment, the scaler's fit and the files app.run writes are the
same.  Every comparison is of bit patterns (`.view(np.int64)`); nothing is tolerated.  Shapes: the smallest at which a point
tile (64), a block of dimensions (64), a slab (CHRONOCLUST_HIP_INGEST_SLAB=128: 1 000 points are 8 slabs, the last partial)
or a chunk of cc_assign is crossed."""
import os

import numpy as np
import pytest

import assign_util as A
import scenarios
import table_util as T
from pipeline_util import knobs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

F32 = np.finfo(np.float32)
# +0.0, -0.0, the smallest and the largest subnormal, FLT_MIN, +-FLT_MAX
SPECIALS = np.array([0.0, -0.0, F32.smallest_subnormal, np.nextafter(F32.tiny, np.float32(0)), F32.tiny, F32.max, -F32.max],
                    dtype=np.float32)
NS = (1, 63, 64, 65, 127, 129, 1000)
DS = (1, 2, 3, 7, 8, 9, 13, 20, 33, 63, 64, 65, 100, 129)
SLABS = (None, 128)


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float64
    return a.view(np.int64)


def same_bits(got, exp, what):
    diff = None if np.array_equal(bits(got), bits(exp)) else T._first_diff(bits(got), bits(exp))
    assert diff is None, "%s: %s" % (what, diff)


def points32(n, d, turn=0):
    """Random float32 [n, d] with a special value at element 0, at the last element and at the last element of the first point
    tile - which special: by `turn`, so that over a grid of cases every one of them stands at every place - and all of them
    scattered over the rest where there is room."""
    rng = np.random.default_rng(1000 * n + d)
    x = rng.uniform(-4.0, 4.0, (n, d)).astype(np.float32)
    flat = x.reshape(-1)
    if flat.size > 40:
        where = rng.choice(np.arange(1, flat.size - 1), 3 * len(SPECIALS), replace=False)
        flat[where] = np.tile(SPECIALS, 3)
    for i, at in enumerate((0, flat.size - 1, min(n, 64) * d - 1)):
        flat[at] = SPECIALS[(turn + i) % len(SPECIALS)]
    return x


@pytest.fixture(scope="module", params=SLABS, ids=lambda s: "slab%s" % s)
def handle(request):
    """One handle per slab setting for the tests that only move points (the knob is read when a handle is created)."""
    from chronoclust_amd import _lib
    env = {} if request.param is None else dict(CHRONOCLUST_HIP_INGEST_SLAB=request.param)
    with knobs(**env):
        h = _lib.Handle(0)
    yield h
    h.close()


def check_resident(h, x32, exp, what):
    """The row-major copy is `exp`, the dimension-major copy its transpose under xt_rows(d) rows, the padded ones +0.0 bits."""
    from chronoclust_amd import _lib
    n, d = x32.shape
    same_bits(h.points_download(d), exp, what + " row-major")
    xt = h.points_download_xt(d)
    assert xt.shape == (_lib.xt_rows(d), n)
    same_bits(xt[:d], exp.T, what + " dimension-major")
    assert not bits(xt[d:]).any(), what + " padded rows"
    return xt


# ---- 1. ingest alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
def test_ingest_alone(handle, n):
    from chronoclust_amd import _lib
    for i, d in enumerate(DS):
        x32 = points32(n, d, turn=NS.index(n) + i)
        wide = x32.astype(np.float64)
        before = handle.stats()["f32_points"]
        handle.points_upload(x32)
        assert handle.stats()["f32_points"] == before + n
        xt32 = check_resident(handle, x32, wide, "float32 %d x %d" % (n, d))
        handle.points_upload(wide)  # the float64 route under the same download: the download is not what is being tested
        assert handle.stats()["f32_points"] == before + n
        xt64 = check_resident(handle, x32, wide, "float64 %d x %d" % (n, d))
        same_bits(xt32, xt64, "the two routes' dimension-major copies, %d x %d" % (n, d))
        assert xt32.shape[0] == (_lib.scan_width(d, False, False)[0] if 8 < d <= 64 else d)


def test_ingest_1024_dimensions(handle):
    x32 = points32(70, 1024, turn=3)
    handle.points_upload(x32)
    check_resident(handle, x32, x32.astype(np.float64), "float32 70 x 1024")


# ---- 2. scaled ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d", [(1, 3), (65, 13), (129, 20), (1000, 9), (127, 64), (129, 129), (70, 1024)])
def test_scaled(handle, n, d):
    from chronoclust_amd.scaling.scaler import Scaler
    x32 = points32(n, d, turn=n + d)
    wide = x32.astype(np.float64)
    sc = Scaler()
    sc.fit_scaler(x32)
    exp = wide * sc.scale_ + sc.min_  # numpy: two roundings per element
    handle.points_upload_scaled(x32, sc.scale_, sc.min_)
    check_resident(handle, x32, exp, "scaled float32 %d x %d" % (n, d))
    handle.points_upload_scaled(wide, sc.scale_, sc.min_)
    check_resident(handle, x32, exp, "scaled float64 %d x %d" % (n, d))


def test_a_scale_that_overflows_is_refused_on_both_routes(handle):
    x32 = np.random.default_rng(5).uniform(1.0, 2.0, (300, 5)).astype(np.float32)
    x32[200, 3] = 1e30
    scale, min_ = np.ones(5), np.zeros(5)
    handle.points_upload_scaled(x32, scale, min_)  # finite as long as the scale leaves it so
    scale[3] = 1e300
    for x in (x32, x32.astype(np.float64)):
        with pytest.raises(ValueError, match="non-finite"):
            handle.points_upload_scaled(x, scale, min_)


# ---- 3. non-finite input ----------------------------------------------------------------------------------------------------

def test_non_finite_input_is_refused_and_leaves_the_handle_sound():
    """300 points in slabs of 128: element 0, the last element, the last partial tile (points 256 ..) and a later slab; from
    the upload, from a prefetch followed by the upload and from assign.  Afterwards the handle clusters a clean array as the
    oracle does, and a refused assign has moved nothing."""
    from chronoclust_amd import _lib
    name = "stale-31+33x5"
    pcores, outliers, par, X = A.case(name)[:4]
    clean = np.ascontiguousarray(np.tile(X, (3, 1))[:300].astype(np.float32))
    n, d = clean.shape
    with knobs(CHRONOCLUST_HIP_INGEST_SLAB=128, CHRONOCLUST_HIP_ASSIGN_CHUNK=128):
        h = _lib.Handle(0)
    try:
        T.fill_handle(h, par, pcores, outliers)
        h.set_tuning(sequential=1)
        h.online(np.ascontiguousarray(clean[:5] + np.float32(100.0)))  # labels to keep: five new outliers

        def snapshot():
            lists = [h.export(kind) for kind in (_lib.PCORE, _lib.OUTLIER)]
            return ([{k: v.tobytes() for k, v in t.items()} for t in lists], h.counters(),
                    tuple(a.tobytes() for a in h.labels_download()))

        before = snapshot()
        for value in (np.nan, np.inf, -np.inf):
            for at in ((0, 0), (n - 1, d - 1), (270, 2), (200, 1)):
                bad = clean.copy()
                bad[at] = value
                with pytest.raises(ValueError, match="non-finite"):
                    h.assign(bad)
                assert snapshot() == before, "a refused assign moved something (%r at %r)" % (value, at)
        h.reset()
        for value in (np.nan, np.inf, -np.inf):
            for at in ((0, 0), (n - 1, d - 1), (270, 2), (200, 1)):
                bad = clean.copy()
                bad[at] = value
                with pytest.raises(ValueError, match="non-finite"):
                    h.points_upload(bad)
                h.points_prefetch(bad)
                with pytest.raises(ValueError, match="non-finite"):
                    h.points_upload(bad)
        # the same handle, a clean array: the oracle's labels and lists, the frozen oracle's answers
        wide = clean.astype(np.float64)
        o = T.make_oracle(par, pcores, outliers)
        o.online_microcluster_maintenance(wide, 0, reset_param=False, offline=False)
        T.fill_handle(h, par, pcores, outliers)
        tables = [T.Table.__new__(T.Table) for _ in range(2)]
        for t, kind in zip(tables, (_lib.PCORE, _lib.OUTLIER)):
            t.__dict__.update(h.export(kind))
        sub = slice(None, None, 7)
        A.same_assign(tuple(g[sub] for g in h.assign(clean, want_dist=True)),
                      A.frozen_answers(tables[0], tables[1], par, wide[sub]), name + " after refused calls")
        T.same_online(h, (h.online(clean), None), dict(o=o, uid=o.labels_uid, path=o.paths), name + " after refused calls")
    finally:
        h.close()


# ---- 4. the online phase does not notice --------------------------------------------------------------------------------------

TIME_FIELDS = ("scan_ms", "run_ms", "comm_ms", "scan_ms_pruned", "calib_allgather_us", "calib_scan_ns_per_row_dim")
# width -> (points, blobs, tuning): 3 k_seq_r, 13 padded operands, 20 / 40 / 64 the ladder, 80 k_seq_g, 200 its wide form.  The
# sequential kernel is switched on (d = 3) or off by tuning where the policy would otherwise decide by the clock.
WIDTHS = {3: (3000, 6, dict(sequential=2)), 13: (3000, 40, dict(sequential=1)), 20: (4000, 200, dict(sequential=1)),
          40: (3000, 40, dict(sequential=1)), 64: (2000, 20, dict(sequential=1)), 80: (2000, 15, {}), 200: (1500, 10, {})}
_streams = {}


def stream32(d):
    """Two timepoints of the blob generator rounded to float32, and the configuration they are clustered with."""
    if d not in _streams:
        n, g, _ = WIDTHS[d]
        over = dict(param_epsilon=0.08, param_k=4, param_pi=3) if d == 3 else (dict(param_epsilon=0.08) if d >= 80 else {})
        cfg = scenarios.params_to_config(scenarios.blob_params(n, **over))
        _streams[d] = (cfg, [np.ascontiguousarray(scenarios.make_blobs(7000 + 10 * d + t, n, d, g, 0.05 if d == 3 else 0.01)
                                                  .astype(np.float32)) for t in range(2)])
    return _streams[d]


def run_stream(cfg, Xs, tuning, device=0, stream=None):
    from chronoclust_amd.clustering.hddstream import HDDStream
    h = stream if stream is not None else HDDStream(cfg, device=device, tuning=tuning or None)
    out = []
    for t, X in enumerate(Xs):
        h.online_microcluster_maintenance(X, t)
        out.append(dict(uid=h.labels_uid.copy(), path=h.labels_path.copy(), tables=[h.table(k) for k in (0, 1)],
                        counters=(h.pcore_MC_last_id, h.outlier_MC_last_id),
                        members=[list(c.members_in_merge_order) for c in h.final_clusters], stats=h.stats(),
                        resident=h.resident_points(), points_of=h._points_of(int(h.labels_uid[0]))))
    return h, out


def same_run(a, b, what):
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


@pytest.mark.parametrize("prune", [2, 0], ids=["pruned_forced", "pruned_forbidden"])
@pytest.mark.parametrize("d", sorted(WIDTHS))
def test_the_online_phase_does_not_notice(d, prune):
    cfg, Xs = stream32(d)
    wide = [x.astype(np.float64) for x in Xs]
    with knobs(CHRONOCLUST_HIP_PRUNE=prune):
        h64, r64 = run_stream(cfg, wide, WIDTHS[d][2])
        h32, r32 = run_stream(cfg, Xs, WIDTHS[d][2])
    same_run(r32, r64, "d=%d" % d)
    for t, (a, b) in enumerate(zip(r32, r64)):
        for key, val in b["stats"].items():
            if key not in TIME_FIELDS and key != "f32_points":
                assert a["stats"][key] == val, "d=%d t=%d cc_stats.%s: %r / %r" % (d, t, key, a["stats"][key], val)
        assert a["stats"]["f32_points"] == sum(len(x) for x in Xs[:t + 1]) and b["stats"]["f32_points"] == 0
    assert r32[0]["resident"].dtype == np.float64 and h32._X.dtype == np.float64  # (widened on demand by _points_of)
    if d == 20:  # two equal wrong answers must not pass: the oracle on the widened values
        from oracle import oracle as O
        o = O.OracleHDDStream(cfg)
        for t, x in enumerate(wide):
            o.online_microcluster_maintenance(x, t)
            assert np.array_equal(r32[t]["uid"], o.labels_uid) and np.array_equal(r32[t]["path"], o.paths)
            for kind in (0, 1):
                for key in T.KEYS:
                    assert np.array_equal(r32[t]["tables"][kind][key], o.table(kind)[key]), (t, kind, key)
            assert r32[t]["members"] == [[int(x) for x in c["members"]] for c in o.clusters]
        if prune == 2:
            assert sum(r["stats"]["scan_p_launches"] for r in r32) > 0  # (x_absmax was read by a pruned scan)


# ---- 5. prefetch --------------------------------------------------------------------------------------------------------------

def test_prefetch(handle):
    from chronoclust_amd.scaling.scaler import Scaler
    n, d = 1000, 13
    x32, other = points32(n, d, turn=1), points32(n, d, turn=4)[::-1].copy()
    wide = x32.astype(np.float64)
    sc = Scaler()
    sc.fit_scaler(x32)
    for scaling in (None, (sc.scale_, sc.min_)):
        exp = wide if scaling is None else wide * scaling[0] + scaling[1]
        upload = handle.points_upload if scaling is None else (lambda x: handle.points_upload_scaled(x, *scaling))
        pre = (lambda x: handle.points_prefetch(x)) if scaling is None else (lambda x: handle.points_prefetch(x, *scaling))
        pre(x32)
        upload(x32)  # adopted
        check_resident(handle, x32, exp, "prefetched float32")
        pre(x32)
        upload(other)  # another array: discarded
        exp_other = other.astype(np.float64) if scaling is None else other.astype(np.float64) * scaling[0] + scaling[1]
        check_resident(handle, other, exp_other, "another array behind a prefetch")
        pre(x32)
        upload(wide)  # a float64 array: discarded
        check_resident(handle, x32, exp, "a float64 array behind a float32 prefetch")
    # scaled prefetch, plain upload of the same array: not this upload
    handle.points_prefetch(x32, sc.scale_, sc.min_)
    handle.points_upload(x32)
    check_resident(handle, x32, wide, "plain upload behind a scaled prefetch")


def test_prefetch_is_matched_on_the_element_type_too(handle):
    """A float32 and a float64 array of one shape at ONE address: neither adopts the other's prefetch."""
    n, d = 300, 6
    buf = np.zeros(n * d, dtype=np.float64)
    x64 = buf.reshape(n, d)
    x32 = buf.view(np.float32)[:n * d].reshape(n, d)
    x32[:] = np.random.default_rng(9).uniform(0.5, 1.5, (n, d)).astype(np.float32)
    assert x32.ctypes.data == x64.ctypes.data and np.isfinite(x64).all()
    handle.points_prefetch(x32)
    handle.points_upload(x64)
    same_bits(handle.points_download(d), x64, "float64 upload behind a float32 prefetch of its address")
    handle.points_prefetch(x64)
    handle.points_upload(x32)
    same_bits(handle.points_download(d), x32.astype(np.float64), "float32 upload behind a float64 prefetch of its address")


# ---- 6. assign ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["victims-k4-600x20", "victims-filter-600x20", "lattice-100+64x200", "stale-filter-150x200"])
def test_assign(name):
    """d = 20 and 200, the pdim filter off and on; n = 0, 1, 64, 100; chunks of 1, 64 and 100 points."""
    from chronoclust_amd import _lib
    pcores, outliers, par, X = T.build_online(name)[:4]
    x32 = np.ascontiguousarray(X[:100].astype(np.float32))
    wide = x32.astype(np.float64)
    assert (par.pi < X.shape[1]) == ("filter" in name)
    for chunk in (None, 1, 64, 100):
        with knobs(**({} if chunk is None else dict(CHRONOCLUST_HIP_ASSIGN_CHUNK=chunk, CHRONOCLUST_HIP_INGEST_SLAB=128))):
            h = _lib.Handle(0)
        try:
            T.fill_handle(h, par, pcores, outliers)
            for n in (0, 1, 64, 100):
                exp = h.assign(wide[:n], want_dist=True)
                launches = h.stats()["assign_launches"]
                got = h.assign(x32[:n], want_dist=True)
                A.same_assign(got, exp, "%s n=%d chunk=%s" % (name, n, chunk))
                same_bits(got[2], exp[2], "%s n=%d chunk=%s dist" % (name, n, chunk))
                assert h.stats()["assign_launches"] == launches == (0 if n == 0 else -(-n // (chunk or n)))
                assert h.stats()["assign_points"] == n
            assert h.stats()["f32_points"] == 165
        finally:
            h.close()


def test_assign_in_a_group_of_two():
    name = "victims-k4-600x20"
    pcores, outliers, par, X = T.build_online(name)[:4]
    x32 = np.ascontiguousarray(X[:200].astype(np.float32))
    parts = [slice(0, 100), slice(100, None)]

    def work(h, rank):
        T.fill_handle(h, par, pcores, outliers)
        return h.assign(x32[parts[rank]], want_dist=True), h.assign(x32[parts[rank]].astype(np.float64), want_dist=True)

    hs, got = T._run_group(2, work)
    try:
        for rank in range(2):
            A.same_assign(got[rank][0], got[rank][1], "%s rank %d of 2" % (name, rank))
            s = hs[rank].stats()
            assert s["comm_launches"] == 0 and s["f32_points"] == 100 and hs[rank].comm_info()["world"] == 2, s
    finally:
        for h in hs:
            h.close()


# ---- 7. col_minmax ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d", [(1, 1), (1, 257), (300, 1), (1000, 20), (700, 256), (700, 257), (520, 1024)])
def test_col_minmax(handle, n, d):
    x32 = points32(n, d, turn=d)
    rng = np.random.default_rng(n + d)
    if n > 1:
        x32[rng.integers(0, n, max(1, n // 10)), rng.integers(0, d, max(1, n // 10))] = np.nan  # some NaN in some columns
        x32[n // 2, 0] = -0.0
        x32[:, d // 2] = np.nan  # an all-NaN column
    wide = x32.astype(np.float64)
    mn32, mx32 = handle.col_minmax(x32)
    mn64, mx64 = handle.col_minmax(wide)
    same_bits(mn32, mn64, "minima, the two routes")
    same_bits(mx32, mx64, "maxima, the two routes")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (numpy warns about the all-NaN column)
        exp_mn, exp_mx = np.nanmin(wide, axis=0), np.nanmax(wide, axis=0)
    some = ~np.isnan(wide).all(axis=0)
    same_bits(mn32[some], exp_mn[some], "minima against np.nanmin")
    same_bits(mx32[some], exp_mx[some], "maxima against np.nanmax")
    assert (mn32[~some] == np.inf).all() and (mx32[~some] == -np.inf).all()  # nothing to reduce: the identities, as on the float64 route
    if n > 1:
        assert (~some).sum() == 1


# ---- 8. app.run -------------------------------------------------------------------------------------------------------------------

def test_app_run_writes_the_same_files(tmp_path, monkeypatch):
    """The bundled d0-d4 data rounded to float32, once as float32 `.npy` and once as float64 `.npy` of the same values:
    result.csv and every cluster_points_D{t}.csv byte for byte; the first run took the single-precision route."""
    import pandas as pd
    from chronoclust_amd import app
    from golden_util import GOLDEN
    from test_app_end_to_end import _reset_logging
    c1 = os.path.join(GOLDEN, "c1")
    made = []

    class Recording(app.HDDStream):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(app, "HDDStream", Recording)
    outs, total = [], 0
    for kind in (np.float32, np.float64):
        files = []
        for t in range(5):
            x = pd.read_csv(os.path.join(c1, "synthetic_d%d.csv.gz" % t)).to_numpy().astype(np.float32)
            fn = os.path.join(str(tmp_path), "tp%d_%s.npy" % (t, np.dtype(kind).name))
            np.save(fn, x.astype(kind))
            files.append(fn)
            total += len(x) if kind is np.float32 else 0
        out = os.path.join(str(tmp_path), "out_" + np.dtype(kind).name)
        os.makedirs(out)
        try:
            app.run(data=files, output_directory=out, **scenarios.C1_PARAMS)
        finally:
            _reset_logging()
        outs.append(out)
    for fn in ["result.csv"] + ["cluster_points_D%d.csv" % t for t in range(5)]:
        a, b = (open(os.path.join(o, fn), "rb").read() for o in outs)
        assert a == b and len(a) > 0, fn
    assert [m.stats()["f32_points"] for m in made] == [total, 0] and total > 0


# ---- 9. a group -------------------------------------------------------------------------------------------------------------------

def test_a_group_of_two_fed_float32():
    from chronoclust_amd import _lib
    name = "stale-3000+1096x20"
    case = T.build_online(name)
    pcores, outliers, par, X, meta = case
    x32 = np.ascontiguousarray(X.astype(np.float32))
    case32 = (pcores, outliers, par, x32, meta)
    h = _lib.Handle(0)
    try:
        single = T.handle_online(h, (pcores, outliers, par, x32.astype(np.float64), meta))
        lists = [h.export(kind) for kind in (0, 1)]
        counters = h.counters()
    finally:
        h.close()
    hs, labels, stats = T.group_online(2, case32)
    try:
        for rank in range(2):
            for key, a, b in (("uid", labels[rank][0][0], single[0][0]), ("path", labels[rank][0][1], single[0][1])):
                diff = T._first_diff(a, b)
                assert diff is None, "rank %d %s: %s" % (rank, key, diff)
            for kind in (0, 1):
                got = hs[rank].export(kind)
                for key in T.KEYS:
                    assert got[key].tobytes() == lists[kind][key].tobytes(), (rank, kind, key)
            assert hs[rank].counters() == counters and stats[rank]["f32_points"] == len(x32)
            assert stats[rank]["sharded_windows"] > 0, stats[rank]
    finally:
        for g in hs:
            g.close()
