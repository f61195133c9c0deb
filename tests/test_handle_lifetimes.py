"""One lived handle against the CPU oracle, bit for bit after every step (tests/lifetime_util.py holds the itineraries).

Almost every other parity test builds a fresh handle - the one state in which nothing can be stale.  Here a handle goes from a
wide table to a narrow one, from a padded width to a ladder width of the same padded size, from the register-resident kernel
to the table-in-HBM kernel to windows, from 10 001 rows to 30, from a 4 096-point window to a 1-point window, through tainted
and clean tables, through k 4 -> 3 -> 0.5 -> 4 and the pdim filter on -> off -> on (section 1, through reset()); whole streams
follow one another on it, forwards and reversed, and a finished stream's state is restored into it behind a stream of another
width (section 2); decay empties its table and another dimensionality follows without a reset, prefetches are adopted,
discarded and left outstanding across read-only calls, a table collapses and regrows across the 10 000-row line (section 3);
and every read-only call is placed between an upload and the run that consumes it (section 4).  No tolerance anywhere; when a
lived step fails, the same step runs on a fresh handle and the message says whether that one agrees with the oracle."""
import numpy as np
import pytest

import assign_util as A
import lifetime_util as L
import table_util as T
import transform_util as U
from pipeline_util import knobs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]


# ---- 1. lives through reset() ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", L.MODE_NAMES)
@pytest.mark.parametrize("life", list(L.LIVES))
def test_life_through_reset(life, mode):
    L.run_life(life, mode)


# ---- 2. whole streams on a lived handle -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", L.MODE_NAMES)
@pytest.mark.parametrize("order", list(L.ORDERS))
def test_streams_follow_one_another_on_one_handle(order, mode):
    L.run_stream_life(order, mode)


# ---- 3. lives without reset() -----------------------------------------------------------------------------------------------

def _online(h, X):
    return h.online(X), None


def _regime(h, mode, n, padded=None):
    """What cc_stats says after a call on an untainted table of a width k_scan_u serves: every point was taken; where the mode
    forbids the sequential kernels the call stayed on the windows, else it ran on one of the two; a call that stayed on the
    windows launched the scalar-operand scan - and k_pad_rows exactly where the width is off the ladder."""
    s = h.stats()
    assert s["points"] == n, s
    if L.MODES[mode][1].get("sequential") == 1:
        assert s["windows"] > 0 and s["seq_points"] == 0, s
    else:
        assert s["windows"] > 0 or s["seq_points"] > 0, s
    if s["seq_points"] == 0:
        assert s["scan_u_launches"] > 0, s
        if padded is not None:
            assert (s["pad_rows_launches"] > 0) == padded, s
    return s


@pytest.mark.parametrize("mode", L.MODE_NAMES)
def test_decay_empties_the_table_and_another_width_follows(mode):
    """d = 20: table, points, offline phase (the cluster lists and creation-number map of this life stay behind); decay until
    nothing is left - the lists against the oracle's after every call -; then points of d = 13 on the same handle, which set_dim
    accepts while no row is held; ids continue."""
    e = L.emptied()
    h = L.new_handle(mode)
    try:
        c = e["first_case"]
        T.same_online(h, T.handle_online(h, c), e["first"], "first life [%s]" % mode)
        T.same_offline(T.handle_offline(h), e["first"]["offline"], "first life offline")
        assert h.counters() == e["first"]["counters"]
        for i, snap in enumerate(e["decays"]):
            h.decay_downgrade(L.EMPTIED_FACTOR)
            T.same_lists(h, snap, "decay %d" % i)
        assert e["decays"][-1].rows() == 0 and h.count(0) == 0 and h.count(1) == 0
        c2 = e["then_case"]
        X = c2[3]
        assert X.shape[1] == 13 and h.dim() == 20
        h.set_params(*c2[2])
        T.same_online(h, _online(h, X), e["then"], "d = 13 behind the emptied d = 20 table [%s]" % mode)
        assert h.dim() == 13
        _regime(h, mode, len(X), padded=True)                    # (13 is padded to 14: the mirror of this life is built)
        T.same_offline(T.handle_offline(h), e["then_offline"], "offline behind the emptied table")
        got = h.point_clusters()
        assert T._first_diff(got, e["then_point_clusters"]) is None, T._first_diff(got, e["then_point_clusters"])
        assert (got >= 0).any() and (got < 0).any()
    finally:
        h.close()


def test_another_width_is_refused_while_rows_are_held():
    """The same change with rows held: "dimensionality differs" from online, assign and every kind of upload; nothing moved."""
    r = L.readonly("clean-2000+1000x20")
    c, X = r["case"], r["X"]
    h = L.new_handle("default")
    try:
        T.fill_handle(h, c[2], c[0], c[1])
        h.points_upload(X)
        held = (h.points_download(20), h.points_download_xt(20))
        lists = [h.export(kind) for kind in (0, 1)]
        counters, before = h.counters(), h.stats()
        other = np.random.default_rng(13).uniform(0.1, 0.9, (300, 13))
        for kind, src in L.sources(other).items():
            for what, call in (("online", h.online), ("assign", h.assign), ("upload", h.points_upload),
                               ("scaled upload", lambda x: h.points_upload_scaled(x, np.ones(13), np.zeros(13)))):
                with pytest.raises(ValueError, match="dimensionality differs"):
                    call(src)
        after = h.stats()
        for key in ("list_points", "view_points", "f32_points", "assign_launches", "assign_points", "scan_launches",
                    "scan_u_launches", "scan_p_launches", "windows", "points", "pad_rows_launches"):
            assert after[key] == before[key], key
        assert h.counters() == counters and h.dim() == 20
        for kind in (0, 1):
            now = h.export(kind)
            for key in T.KEYS:
                assert T._first_diff(now[key], lists[kind][key]) is None, (kind, key)
        U.same_bits(h.points_download(20), held[0], "resident points behind refused calls")
        U.same_bits(h.points_download_xt(20), held[1], "resident points behind refused calls, dimension-major")
        # and the run consumes the upload as if nothing had been asked
        h.set_counters(*L.HIGH_COUNTERS)
        h.online_run()
        T.same_online(h, (h.labels_download(), None), r["exp"], "run behind the refusals")
    finally:
        h.close()


@pytest.mark.parametrize("mode", L.MODE_NAMES)
@pytest.mark.parametrize("d", [16, 20])
def test_timepoint_sizes_with_prefetch(d, mode):
    """20 000 -> 1 -> 3 000 -> 64 -> 20 000 points on one stream.  d = 16: float32 timepoints, every one prefetched, and the upload
    adopts it - prefetch() hands back the very array and cc_f32_points counts it, so nothing copied it on the way; d = 20: a
    decoy of the same shape, or the very array under a scaling, is prefetched and the upload of the real array discards it.
    The next prefetch is outstanding while the offline phase and an association run."""
    from oracle import oracle as O
    from test_hip_parity import _check_against_oracle
    cfg, Xs, decoys, snaps = L.prefetch_stream(d)
    h = L.new_handle(mode)
    s = L.adopt(h, cfg)
    try:
        ahead = Xs if d == 16 else decoys
        assert s.prefetch(ahead[0]) is ahead[0]
        for t, X in enumerate(Xs):
            if d == 16:                                          # what was prefetched is what is uploaded, as it lies
                assert h._prefetched[0] is X and X.dtype == np.float32
            taken = h.f32_points()
            s.online_microcluster_maintenance(X, t)
            assert h._prefetched is None
            assert h.f32_points() - taken == (len(X) if d == 16 else 0)
            _check_against_oracle(s, snaps[t])
            _regime(h, mode, len(X), padded=False)
            if t + 1 < len(Xs):
                if d == 20 and t % 2:                            # the very array of the next upload, but under a scaling
                    s.prefetch(Xs[t + 1], device_scaling=(np.full(d, 2.0), np.full(d, 0.5)))
                else:
                    assert s.prefetch(ahead[t + 1]) is ahead[t + 1]
                assert h._prefetched is not None
            s.offline_clustering(t)                              # with the prefetch outstanding
            cur = snaps[t].table(0)
            prev = snaps[t - 1].table(0)["cen"] if t else cur["cen"][::-1]
            gi, gd = h.assoc_argmin(cur["cen"], cur["pref"], prev)
            oi, od = O.assoc_argmin(cur["cen"], cur["pref"], prev)
            assert np.array_equal(gi, oi) and np.array_equal(gd, od)
            s._tables = {}                                       # (exported again)
            _check_against_oracle(s, snaps[t])
            U.same_bits(h.points_download(d), X.astype(np.float64), "resident points of timepoint %d" % t)
    finally:
        h.close()


@pytest.mark.parametrize("mode", ["prune2", "default"])
def test_collapse_and_regrowth_across_ten_thousand_rows(mode):
    """An empty table grows past 10 000 rows within one call, three decays delete most of it, 500 points, then regrowth past
    10 000 again - no reset in between."""
    c = L.collapse()
    rows = c["rows"]
    assert rows[0] > 10000 and rows[1] < rows[0] // 4 and rows[2] < 10000 < rows[3], rows
    h = L.new_handle(mode)
    try:
        h.set_params(*L.COLLAPSE_PAR)
        for t, X in enumerate(c["Xs"]):
            if t == 1:
                for _ in range(L.COLLAPSE["decays"]):
                    h.decay_downgrade(L.COLLAPSE["factor"])
                assert h.count(0) + h.count(1) == rows[1]
            T.same_online(h, _online(h, X), c["calls"][t], "collapse call %d [%s]" % (t, mode))
            s = _regime(h, mode, len(X), padded=False)
            if mode == "prune2":
                assert s["scan_p_launches"] > 0, s
            if t == 1:
                T.same_offline(T.handle_offline(h), c["offline"], "offline after the collapse")
    finally:
        h.close()


# ---- 4. read-only calls are read-only -----------------------------------------------------------------------------------------

def _table_of(t):
    return (t["cf1"], t["cf2"], t["cen"], t["pref"], t["w"], t["id"], t["uid"])


def _interposed(h, ref, r, what, d, offline_want):
    """Every read-only call on h - which holds an upload the next run consumes, or labels the offline phase reads - against
    the same call on `ref`, a handle of its own with the same table and the same resident points."""
    Q, X = r["Q"], r["X"]
    src_h, src_ref = L.sources(Q), L.sources(Q)
    for kind in src_h:
        got, want = h.col_minmax(src_h[kind]), ref.col_minmax(src_ref[kind])
        U.same_bits(np.stack(got), np.stack(want), "%s col_minmax %s" % (what, kind))
        A.same_assign(h.assign(src_h[kind], want_dist=True), ref.assign(src_ref[kind], want_dist=True), "%s assign %s" % (what, kind))
    assert h.stats()["assign_points"] == len(Q)
    cur = h.export(0)
    prev = np.ascontiguousarray(Q[:97])
    gi, gd = h.assoc_argmin(cur["cen"], cur["pref"], prev)
    ri, rd = ref.assoc_argmin(cur["cen"], cur["pref"], prev)
    assert np.array_equal(gi, ri) and np.array_equal(gd, rd), what
    scale, mn = np.linspace(0.5, 2.0, d), np.linspace(-0.25, 0.25, d)
    U.same_bits(h.points_download(d), X, what + " points_download")
    U.same_bits(h.points_download(d, scale, mn), ref.points_download(d, scale, mn), what + " points_download, inverse scaling")
    U.same_bits(h.points_download_xt(d), ref.points_download_xt(d), what + " points_download_xt")
    for kind in (0, 1):
        a, b = h.export(kind), ref.export(kind)
        assert h.count(kind) == ref.count(kind)
        for key in T.KEYS:
            assert T._first_diff(a[key], b[key]) is None, (what, kind, key)
    assert h.counters() == ref.counters()
    h.stats()
    for _ in range(2):
        T.same_offline(T.handle_offline(h), offline_want, what + " offline")
    h.points_prefetch(np.random.default_rng(3).random((777, d + 5)))     # unrelated, never uploaded


@pytest.mark.parametrize("chunked", [False, True], ids=["plain", "assign-chunk-100-ingest-slab-64"])
@pytest.mark.parametrize("name", list(L.READONLY))
def test_read_only_calls_between_upload_and_run(name, chunked):
    r = L.readonly(name)
    c, X = r["case"], r["X"]
    d = X.shape[1]
    with knobs(**(dict(CHRONOCLUST_HIP_ASSIGN_CHUNK=100, CHRONOCLUST_HIP_INGEST_SLAB=64) if chunked else {})):
        h = L.new_handle("default")
    ref = L.new_handle("default")
    try:
        for x in (h, ref):
            T.fill_handle(x, c[2], c[0], c[1])
            x.set_counters(*L.HIGH_COUNTERS)
            x.points_upload(X)
        _interposed(h, ref, r, "%s between upload and run" % name, d, r["offline_before"])
        h.online_run()
        T.same_online(h, (h.labels_download(), None), r["exp"], "%s: the run behind the read-only calls" % name)
        s = h.stats()
        assert s["points"] == len(X), s
        # the reference handle: the table the run left, injected; the same resident points
        ref.reset()
        ref.set_params(*c[2])
        for kind in (0, 1):
            t = r["exp"]["o"].table(kind)
            if len(t["id"]):
                ref.inject_bulk(kind, *_table_of(t))
        ref.set_counters(*r["exp"]["o"].counters)
        ref.points_upload(X)
        _interposed(h, ref, r, "%s between run and offline" % name, d, r["offline"])
        T.same_lists(h, r["exp"]["o"], "%s after the second round of read-only calls" % name)
        got = h.point_clusters()
        assert T._first_diff(got, r["point_clusters"]) is None, T._first_diff(got, r["point_clusters"])
        assert (got >= 0).any()
        T.same_offline(T.handle_offline(h), r["offline"], "%s offline at the end" % name)
    finally:
        h.close()
        ref.close()
