"""Kernel timing by device clock stamps (time_kernels = 1): an in-place snapshot scan is timed by two
stamps of the device's constant clock, taken inside the chain's first kernel and k_decide, instead of two event records on
the stream.  Timing must change nothing but the time fields: every case below runs a seeded stream with time_kernels = 0 and,
behind a reset of the same handle, with time_kernels = 1, and compares labels, both tables and every cc_stats field that is
not a time or a count of timed launches; the timed run's scan time must be a time (positive, below the call's own run time)
and its launch counts those of the scans the host enqueued.  (cc_stats are those of the last call.)"""
import numpy as np
import pytest

import scenarios
from pipeline_util import knobs

pytestmark = pytest.mark.gpu

TIME_FIELDS = ("scan_ms", "run_ms", "comm_ms", "scan_ms_pruned", "calib_allgather_us", "calib_scan_ns_per_row_dim")
# counts of TIMED launches: zero by definition with time_kernels = 0, checked on their own below
TIMED_COUNTS = ("scan_launches", "scan_launches_pruned", "comm_launches")
KEYS = ("id", "uid", "w", "cf1", "cf2", "cen", "pref")
STAMP_SLOTS = 64  # CC_STAMP_SLOTS (cc_common.h): window `seq` stamps slot seq % 64


def set_params(h, n, d, k=4.0, pi=0, epsilon=0.05):
    """The blob configuration (scenarios.blob_params) as derived parameters, with the reference's expressions."""
    p = scenarios.params_to_config(scenarios.blob_params(n, param_epsilon=epsilon, param_k=k, param_pi=pi))
    ups = p["upsilon"] * p["epsilon"]
    h.set_params(p["epsilon"] ** 2, p["delta"] ** 2, float(p["k"]), p["beta"], p["mu"] * n, 0.0, ups, ups ** 2, p["delta"],
                 d if p["pi"] <= 0 else int(p["pi"]))


def snapshot(h):
    from chronoclust_amd import _lib
    uid, path = h.labels_download()
    return dict(uid=uid, path=path, tables=[h.export(k) for k in (_lib.PCORE, _lib.OUTLIER)], counters=h.counters(),
                stats=h.stats())


def calls(X, timings, env=None, group=False, k=4.0, epsilon=0.05, **tuning):
    """One handle, one call of the online phase over X per entry of `timings` (time_kernels of that call), each from an empty
    table: the results of every call."""
    from chronoclust_amd import _lib
    tun = dict(dict(window=256, windows_per_sync=4, sequential=1), **tuning)  # (sequential = 1: never the sequential kernel)
    with knobs(**(env or {})):
        h = _lib.Handle(0)
    try:
        if group:  # a group of one rank whose scans are "split" whatever the table's size: the merge + all-gather path
            h.comm_init_rccl(_lib.comm_unique_id(), 0, 1)
            h.set_shard_thresholds(0, 0)
        set_params(h, X.shape[0], X.shape[1], k=k, epsilon=epsilon)
        h.points_upload(X)
        out = []
        for time_kernels in timings:
            h.set_tuning(time_kernels=time_kernels, **tun)
            h.reset()
            h.online_run()
            out.append(snapshot(h))
        if group:
            h.comm_destroy()
        return out
    finally:
        h.close()


def same_results(a, b, what):
    for key in ("uid", "path"):
        assert np.array_equal(a[key], b[key]), "%s: %s per point differs" % (what, key)
    for kind in (0, 1):
        for key in KEYS:
            assert a["tables"][kind][key].tobytes() == b["tables"][kind][key].tobytes(), (what, kind, key)
    assert a["counters"] == b["counters"], what
    for key, val in b["stats"].items():
        if key not in TIME_FIELDS and key not in TIMED_COUNTS:
            assert a["stats"][key] == val, "%s cc_stats.%s: %r / %r" % (what, key, a["stats"][key], val)


def timed_is_sane(on, off, what, single_stream_common=True):
    s, s0 = on["stats"], off["stats"]
    print("%s: windows %d scan_launches %d (pruned %d) scan_ms %.4f (pruned %.4f) run_ms %.4f lookahead_windows %d" % (
        what, s["windows"], s["scan_launches"], s["scan_launches_pruned"], s["scan_ms"], s["scan_ms_pruned"], s["run_ms"],
        s["lookahead_windows"]))
    assert s0["scan_launches"] == 0 and s0["scan_ms"] == 0.0 and s0["scan_launches_pruned"] == 0 and s0["scan_ms_pruned"] == 0.0, what
    assert 0.0 < s["scan_ms"] < s["run_ms"], (what, s["scan_ms"], s["run_ms"])
    assert 0.0 <= s["scan_ms_pruned"] <= s["scan_ms"], (what, s["scan_ms_pruned"], s["scan_ms"])
    assert s["scan_launches_pruned"] <= s["scan_launches"]
    assert (s["scan_ms_pruned"] > 0.0) == (s["scan_launches_pruned"] > 0), what
    # every window that ran had a scan enqueued for it; where the rows are scalar operands (k a power of two, no pdim filter)
    # the library counts every enqueued snapshot scan, timed or not, as scan_u_launches: the timed count must be that one
    assert s["scan_launches"] >= s["windows"], what
    if single_stream_common:
        assert s["scan_launches"] == s0["scan_u_launches"] == s["scan_u_launches"], (what, s["scan_launches"], s0["scan_u_launches"])
        assert s["scan_launches_pruned"] == s["scan_p_launches"], what


def on_against_off(X, what, single_stream_common=True, **kw):
    off, on = calls(X, (0, 1), **kw)
    same_results(on, off, what)
    timed_is_sane(on, off, what, single_stream_common)
    return on["stats"], off["stats"]


_cache = {}


def blobs(n, d, g=40):
    if (n, d, g) not in _cache:
        _cache[(n, d, g)] = scenarios.make_blobs(9100 + d, n, d, g)
    return _cache[(n, d, g)]


@pytest.mark.parametrize("d,lookahead", [(4, 0), (20, 0), (4, 2)], ids=["d4", "d20", "d4_in_place_throughout"])
def test_timing_on_against_off(d, lookahead):
    """80 windows of 256 points, four per batch: the ring of stamp slots wraps and the windows' parities alternate.
    (lookahead 0: the policy's choice, which at d = 4 is lookahead scans for most windows; 2: every scan in place.)"""
    s, _ = on_against_off(blobs(20480, d), "d=%d lookahead=%d" % (d, lookahead), lookahead=lookahead)
    assert s["windows"] > STAMP_SLOTS, "the stream must wrap the ring of stamp slots"
    if lookahead == 2:
        assert s["lookahead_windows"] == 0


# name -> (d, environment, k, what the statistics of the run must show): every kernel that can be the first of an in-place chain
FORMS = {
    "plain scan": (20, dict(CHRONOCLUST_HIP_PRUNE=0), 4.0, lambda s: s["scan_u_launches"] > 0 and s["scan_p_launches"] == 0),
    "seeded chain": (20, dict(CHRONOCLUST_HIP_PRUNE=2, CHRONOCLUST_HIP_GUESS=0), 4.0,
                     lambda s: s["scan_p_launches"] > 0 and s["scan_g_launches"] == 0 and s["seed16_launches"] == 0),
    "guessed thresholds": (20, dict(CHRONOCLUST_HIP_PRUNE=2), 4.0, lambda s: s["scan_g_launches"] > 0),
    "guessed thresholds, prefix test on the VALU": (20, dict(CHRONOCLUST_HIP_PRUNE=2, CHRONOCLUST_HIP_SCANP3=0), 4.0,
                                                    lambda s: s["scan_g_launches"] > 0),
    "guessed thresholds, one point per lane": (20, dict(CHRONOCLUST_HIP_PRUNE=2, CHRONOCLUST_HIP_SCANP3=0, CHRONOCLUST_HIP_SCANP2=0), 4.0,
                                               lambda s: s["scan_g_launches"] > 0),
    "guessed thresholds, split phases": (20, dict(CHRONOCLUST_HIP_PRUNE=2, CHRONOCLUST_HIP_SCANA=2), 4.0,
                                         lambda s: s["scan_g_launches"] > 0),
    "padded width": (13, dict(CHRONOCLUST_HIP_PRUNE=2), 4.0, lambda s: s["pad_rows_launches"] > 0 and s["scan_p_launches"] > 0),
    "general chain": (20, dict(CHRONOCLUST_HIP_PRUNE=2), 3.0, lambda s: s["scan_u_launches"] == 0 and s["scan_p_launches"] > 0),
    "general scan": (20, dict(CHRONOCLUST_HIP_PRUNE=0), 3.0, lambda s: s["scan_u_launches"] == 0 and s["scan_p_launches"] == 0),
    "seeds from the matrix cores": (20, dict(CHRONOCLUST_HIP_PRUNE=2, CHRONOCLUST_HIP_GUESS=0, CHRONOCLUST_HIP_SEED16=1), 4.0,
                                    lambda s: s["seed16_launches"] > 0),
}
FORM_POINTS = 4096  # sixteen windows of 256 points: four batches, both window parities, in place throughout


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_first_kernel_form(form):
    d, env, k, ran = FORMS[form]
    s, _ = on_against_off(blobs(FORM_POINTS, d), form, single_stream_common=(k == 4.0), env=env, k=k, lookahead=2)
    assert ran(s), (form, s)
    if k != 4.0:  # (no scan_u_launches there: one scan per window that ran, this stream idles no batch)
        assert s["scan_launches_pruned"] == s["scan_p_launches"]


def test_lookahead_scans_keep_their_events():
    s, _ = on_against_off(blobs(20480, 20), "lookahead=3", lookahead=3)
    assert s["lookahead_windows"] > 0


def test_split_scans_keep_their_events():
    s, s0 = on_against_off(blobs(FORM_POINTS, 20), "group of one, split forced", single_stream_common=False, group=True, lookahead=2)
    assert s["sharded_windows"] > 0
    assert 0 < s["comm_launches"] <= s["scan_launches"] and s["comm_ms"] > 0.0 and s0["comm_launches"] == 0


def test_one_handle_several_calls():
    """Timing on, off, on, off, each call behind a reset of the one handle: a timed call's scan_ms is a sum of intervals inside
    that call - below its own run time; a stamp left by an earlier call would make it an interval of seconds -, an untimed
    call's is zero, and all four calls give the same results."""
    a, b, c, e = calls(blobs(FORM_POINTS, 20), (1, 0, 1, 0), lookahead=2)
    for r in (a, b, c, e):
        s = r["stats"]
        print("windows %d scan_launches %d scan_ms %.4f run_ms %.4f" % (s["windows"], s["scan_launches"], s["scan_ms"], s["run_ms"]))
    same_results(a, b, "first timed call against the untimed one behind it")
    same_results(c, b, "second timed call against the untimed one before it")
    same_results(c, e, "second timed call against the untimed one behind it")
    timed_is_sane(a, b, "first timed call")
    timed_is_sane(c, e, "second timed call")


def test_a_stalled_batch():
    """A quiet stretch (the host stops launching the dirty scans), then new populations in the middle of a batch (the recipe
    of test_hip_parity.py::test_quiet_stream_then_new_populations, scans in place throughout): a window is cut at a point
    that needs those scans, the next one starts there and commits nothing, and the device idles the rest of the batch.  The
    windows that did not run were enqueued - scan_launches counts them - and left no begin stamp: they add nothing, the scan
    time stays a sum of intervals inside the call."""
    d, g = 8, 30
    rng = np.random.default_rng(77)
    centres = rng.uniform(0.1, 0.9, (g + 6, d))

    def stretch(n, which, sigma=0.01):
        lab = rng.choice(which, n)
        return np.clip(centres[lab] + rng.normal(0.0, sigma, (n, d)), 0.0, 1.0)

    X = np.ascontiguousarray(np.concatenate([stretch(4000, np.arange(g)), stretch(400, np.arange(g, g + 3)),
                                             stretch(2000, np.arange(g + 3)), stretch(600, np.arange(g + 6))]))
    s, _ = on_against_off(X, "stalled batch", epsilon=0.06, lookahead=2, windows_per_sync=16)
    assert s["lookahead_windows"] == 0
    assert s["scan_launches"] > s["windows"], "no batch of this stream was idled: the recipe no longer stalls one"
