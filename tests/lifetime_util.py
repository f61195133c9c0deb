"""One handle, many lives: the itineraries and helpers of tests/test_handle_lifetimes.py (GPU) and
tests/test_handle_lifetimes_cpu.py (what the itineraries contain, no GPU).

A _lib.Handle keeps, through cc_reset and between calls, every buffer it ever sized (window, carry and version buffers, the
scan copies, the padded mirrors, the half-precision row records, masks, the sequential kernels' images, the table store
with its touch stamps), the lookahead fields of Ctl, the resident points, an outstanding prefetch, the offline results and
the association scratch.  "Results never depend on any of this"  is what these lives referee: a handle
is led through tables and streams in an order where each step shrinks something its predecessor left large - width,
padded width, rows, window, k, the pdim filter - and the CPU oracle is compared bit for bit after every step
(table_util.same_online / same_offline, test_hip_parity._check_against_oracle, oracle.assoc_argmin).  When a lived step
fails, the same step runs on a fresh handle and the assertion says whether that one agrees with the oracle: "a leak" or "a
bug of that case".

No step is conditional on the mode: LIVES[life][mode] is an explicit list for every mode of MODES."""
import math

import numpy as np

import table_util as T
from test_online_tables import MODES as ALL_MODES
from test_online_tables import WINDOW_MAX_DIM, _check_stats, _handle

MODE_NAMES = ("prune2", "default", "sequential1")
MODES = {m: ALL_MODES[m] for m in MODE_NAMES}

# ---- new table cases (NOT part of table_util.ONLINE_TABLES: the reference surface enumerates that) -------------------------
# all `stale(..., clean=True)`: entries of k or 1 only, the handle stays untainted and takes the scans of the common case.
# rows x points <= 600 000 each.
LIFE_TABLES = {
    "clean-400+200x64": (T.stale, dict(seed=401, m_p=400, m_o=200, d=64, n=600, clean=True)),
    "clean-300+150x13": (T.stale, dict(seed=402, m_p=300, m_o=150, d=13, n=500, clean=True)),
    "clean-200+100x14": (T.stale, dict(seed=403, m_p=200, m_o=100, d=14, n=400, clean=True)),
    "clean-120+60x63": (T.stale, dict(seed=404, m_p=120, m_o=60, d=63, n=300, clean=True)),
    "clean-60+30x20": (T.stale, dict(seed=405, m_p=60, m_o=30, d=20, n=200, clean=True)),
    "clean-100+50x13": (T.stale, dict(seed=416, m_p=100, m_o=50, d=13, n=300, clean=True)),
    "clean-20+12x2": (T.stale, dict(seed=417, m_p=20, m_o=12, d=2, n=200, clean=True)),
    "clean-60+40x256": (T.stale, dict(seed=418, m_p=60, m_o=40, d=256, n=150, clean=True)),
    "clean-20+14x3": (T.stale, dict(seed=406, m_p=20, m_o=14, d=3, n=300, clean=True)),
    "clean-7001+3000x20-p56": (T.stale, dict(seed=407, m_p=7001, m_o=3000, d=20, n=56, clean=True)),
    "clean-18+12x20": (T.stale, dict(seed=408, m_p=18, m_o=12, d=20, n=200, clean=True)),
    "clean-k3-600+300x20": (T.stale, dict(seed=409, m_p=600, m_o=300, d=20, n=600, k=3.0, clean=True)),
    "clean-k0.5-500+250x20": (T.stale, dict(seed=410, m_p=500, m_o=250, d=20, n=500, k=0.5, clean=True)),
    "clean-k4-300+150x20": (T.stale, dict(seed=411, m_p=300, m_o=150, d=20, n=400, clean=True)),
    "clean-500+250x14": (T.stale, dict(seed=412, m_p=500, m_o=250, d=14, n=600, clean=True)),
    "clean-filter-300+150x14": (T.stale, dict(seed=413, m_p=300, m_o=150, d=14, n=500, clean=True, filt=True)),
    "clean-400+200x32": (T.stale, dict(seed=414, m_p=400, m_o=200, d=32, n=500, clean=True)),
    "clean-200+100x32": (T.stale, dict(seed=415, m_p=200, m_o=100, d=32, n=300, clean=True)),
}
MAX_ROWS_POINTS = 600_000


def build(name):
    gen, kw = LIFE_TABLES[name] if name in LIFE_TABLES else T.ONLINE_TABLES[name]
    return gen(**kw)


def rows_of(case):
    return sum(len(t) for t in case[:2] if t is not None)


_cases = {}


def case(name):
    """(case, the oracle's online result, the oracle's offline result on the table the online call left): built once."""
    if name not in _cases:
        c = build(name)
        exp = T.oracle_online(c)
        T.check_online(c, exp)
        _cases[name] = (c, exp, T.oracle_offline(exp["o"]))
    return _cases[name]


def dims(name):
    gen, kw = LIFE_TABLES[name] if name in LIFE_TABLES else T.ONLINE_TABLES[name]
    return kw["d"]


def params(name):
    """(d, filter on, k a power of two, k, tainted) of a table case without building it twice."""
    c = case(name)[0]
    par, d = c[2], c[3].shape[1]
    return d, par.pi < d, math.frexp(par.k)[0] == 0.5, par.k, bool(c[4]["tainted"])


# ---- 1. lives through reset() ---------------------------------------------------------------------------------------------

def step(name, stats=None, **tuning):
    """One step of a life: the table case, what set_tuning changes in front of it (the rest of the tuning stays what the
    life's earlier steps made it), and the mode _check_stats judges it by where that is not the life's own."""
    return dict(case=name, tuning=tuning, stats=stats)


def _same(steps):
    return {m: steps for m in MODE_NAMES}


# widths: every band in an order where each step is narrower in something than its predecessor left the handle - 64 (ladder) ->
# 13 (padded to 14: pad_stride kept from nothing, then) -> 14 (ladder, the DP of the mirror just used) -> 63 (padded to 64) ->
# 20; the row counts fall all the way, so that half-precision records and scan copies of the earlier table lie beyond m_rows
# - and 13 again right behind 63: pad_stride is that of DP 64 while DP is 14
_WIDTHS = [step("clean-400+200x64", window=4096), step("clean-300+150x13"), step("clean-200+100x14"), step("clean-120+60x63"),
           step("clean-100+50x13"), step("clean-60+30x20")]

# the bands the other lives enter from one side only: d 3 and d 8 with a narrower predecessor, d 200 (behind d 256: the wide
# form of k_seq_g with images and window buffers of a wider life), d 80 and d 20 with a wider one
_BANDS = [step("clean-20+12x2", window=4096), step("clean-20+14x3"), step("lattice-128+127x8"), step("clean-60+40x256"),
          step("lattice-100+64x200"), step("lattice-200+100x80"), step("clean-60+30x20"), step("lattice-64+40x5")]

# regimes: 1 500 rows at d 40 (windows) -> 34 rows at d 3 (k_seq_r where the sequential kernels are allowed) -> d 80 (k_seq_g) ->
# d 200 (its wide form) -> d 8 (k_scan stages for itself) -> 10 001 rows at d 20 (listed / split forms) -> 30 rows at d 20.
# The window stays at 4 096: ensure_window_buffers sizes by the largest window and the largest d the handle has seen.
_REGIMES_WINDOWS = [step("lattice-1000+500x40", window=4096), step("clean-20+14x3"), step("lattice-200+100x80"),
                    step("lattice-100+64x200"), step("lattice-128+127x8"), step("clean-7001+3000x20-p56"),
                    step("clean-18+12x20")]


def _regimes_default():
    """The default mode leaves the choice of a sequential kernel to a timed policy: the d 3 step forces it (sequential=2) and
    the step after it gives the choice back."""
    steps = [dict(s) for s in _REGIMES_WINDOWS]
    steps[1] = step("clean-20+14x3", stats="sequential2", sequential=2)
    steps[2] = step("lattice-200+100x80", sequential=0)
    return steps


# k: 4 -> 3 -> 0.5 -> 4 at one width (Ctl::pow2, inv_k, the GENERAL chain)
_K = [step("clean-2000+1000x20", window=4096), step("clean-k3-600+300x20"), step("clean-k0.5-500+250x20"),
      step("clean-k4-300+150x20")]

# the pdim filter on -> off -> on at one width, lookahead scans forced (only they read the scan copies, whose cf1 / cf2 / w
# are ensured only while the filter is on), windows of 64 points so that every table sees several
_FILTER = [step("clean-filter-1000+500x14", window=64, lookahead=3), step("clean-500+250x14"), step("clean-filter-300+150x14"),
           step("clean-200+100x14"), step("clean-filter-1000+500x14")]

# a tainted table between two clean ones at d = 32 (the existing test of this kind lives at d = 20)
_TAINT = [step("clean-400+200x32", window=4096), step("victims-k4-1000x32"), step("lattice-500+250x32"),
          step("victims-filter-k3-300x32"), step("clean-200+100x32")]

# set_tuning between steps: window 4 096 -> 64 -> 1 -> 1 024, lookahead 3 -> 2 -> 0, windows_per_sync 4 -> 1
_TUNING = [step("clean-2000+1000x20", window=4096, lookahead=3, windows_per_sync=4),
           step("lattice-3000+1096x20", window=64, lookahead=2, windows_per_sync=1),
           step("clean-18+12x20", window=1, lookahead=0),
           step("clean-k3-600+300x20", window=1024),
           step("clean-60+30x20", window=64, lookahead=3, windows_per_sync=4)]

LIVES = {
    "widths": _same(_WIDTHS),
    "bands": _same(_BANDS),
    "regimes": {"prune2": _REGIMES_WINDOWS, "default": _regimes_default(), "sequential1": _REGIMES_WINDOWS},
    "k": _same(_K),
    "filter": _same(_FILTER),
    "taint": _same(_TAINT),
    "tuning": _same(_TUNING),
}


def new_handle(mode):
    return _handle(*MODES[mode])


def tuning_at(mode, steps, i):
    """The tuning in force at step i of a life: the mode's own, then every step's changes up to i."""
    cur = dict(MODES[mode][1])
    for s in steps[:i + 1]:
        cur.update(s["tuning"])
    return cur


_assoc = {}


def assoc_inputs(life, mode, i):
    """(current centroids, their preference vectors, previous centroids) of step i: the pcore list the oracle holds after the
    step against that of the step before it where the width is the same, against random centroids where it changed."""
    steps = LIVES[life][mode]
    name = steps[i]["case"]
    prev_name = steps[i - 1]["case"] if i else None
    key = (prev_name, name)
    if key not in _assoc:
        from oracle import oracle as O
        cur = case(name)[1]["o"].table(0)
        d = cur["cen"].shape[1]
        prev = case(prev_name)[1]["o"].table(0)["cen"] if prev_name and dims(prev_name) == d else None
        if prev is None or len(prev) == 0:
            prev = np.random.default_rng(len(name) + d).uniform(0.1, 0.9, (37, d))
        exp = O.assoc_argmin(cur["cen"], cur["pref"], prev) if len(cur["cen"]) else None
        _assoc[key] = (cur["cen"], cur["pref"], prev, exp)
    return _assoc[key]


def check_regime(name, mode, stats_mode, tuning, s):
    """What cc_stats says about the kernels the step exists for."""
    c = case(name)[0]
    n, d = c[3].shape
    _check_stats(c, stats_mode or mode, s)
    if d > WINDOW_MAX_DIM:
        assert s["windows"] == 0 and s["seq_g_points"] == n, s
        return
    if stats_mode == "sequential2":
        if d <= 4:
            assert s["seq_r_points"] > 0, s
        return
    if tuning.get("sequential") == 1:
        assert s["windows"] > 0 and s["seq_points"] == 0, s
        if tuning.get("window"):
            assert s["windows"] >= -(-n // tuning["window"]), (tuning, s)
        check_mirror(name, s)
        if tuning.get("lookahead") == 3 and tuning.get("window") and n >= 3 * tuning["window"]:
            assert s["lookahead_windows"] > 0, (tuning, s)      # (only lookahead scans read the scan copies)
        if tuning.get("lookahead") == 2:
            assert s["lookahead_windows"] == 0, (tuning, s)


def check_mirror(name, s):
    """k_pad_rows builds the padded mirror in front of every scan of an untainted table whose width is off the ladder, and
    nowhere else (a call that stays on the windows)."""
    d, _, _, _, tainted = params(name)
    dp, scan_u, _ = scan_rule(name)
    padded = 8 < d <= WINDOW_MAX_DIM and scan_u and dp != d and not tainted      # (up to 8 dimensions k_scan pads for itself)
    assert (s["pad_rows_launches"] > 0) == padded, (name, d, dp, s)


def run_step(h, life, mode, i):
    """Step i of a life on handle h: reset, tuning, the table, the points; labels, lists and counters, the offline phase and one
    association against the oracle; the regime from the statistics."""
    steps = LIVES[life][mode]
    st = steps[i]
    name = st["case"]
    c, exp, exp_off = case(name)
    what = "%s[%s] step %d %s" % (life, mode, i, name)
    tuning = tuning_at(mode, steps, i)
    h.reset()
    h.set_tuning(**tuning)
    labels = T.handle_online(h, c)
    s = h.stats()
    T.same_online(h, labels, exp, what)
    check_regime(name, mode, st["stats"], tuning, s)
    T.same_offline(T.handle_offline(h), exp_off, what + " offline")
    cen, pref, prev, want = assoc_inputs(life, mode, i)
    if want is not None:
        gi, gd = h.assoc_argmin(cen, pref, prev)
        diff = T._first_diff(gi, want[0]) or T._first_diff(gd, want[1])
        assert diff is None, "%s assoc_argmin (library / oracle): %s" % (what, diff)
    T.same_lists(h, exp["o"], what + " after the read-only calls")


def located(lived, fresh, what):
    """Runs lived(); when it fails, runs fresh() - the same step on a handle of its own - and says in the assertion whether
    that one agrees with the oracle."""
    try:
        lived()
    except AssertionError as e:
        try:
            fresh()
            verdict = "a FRESH handle agrees with the oracle on this step: state leaked from the handle's earlier life"
        except AssertionError as e2:
            verdict = "a fresh handle fails this step too (a bug of the case, not a leak): %s" % (str(e2).splitlines() or [""])[0]
        raise AssertionError("%s\n%s: %s" % (e, what, verdict)) from e


def run_life(life, mode):
    h = new_handle(mode)
    try:
        for i in range(len(LIVES[life][mode])):
            def fresh(i=i):
                f = new_handle(mode)
                try:
                    run_step(f, life, mode, i)
                finally:
                    f.close()
            located(lambda: run_step(h, life, mode, i), fresh, "%s[%s] step %d" % (life, mode, i))
    finally:
        h.close()


# ---- what the CPU module asserts about the itineraries ----------------------------------------------------------------------

def scan_rule(name):
    """(padded width, k_scan_u serves, chain) of a table case by cc::scan_width - the library's own statement."""
    from chronoclust_amd import _lib
    d, filt, pow2, _, _ = params(name)
    return _lib.scan_width(d, filt, pow2) if d <= WINDOW_MAX_DIM else (d, False, "none")


def band(d):
    """The band of widths a table or stream falls into: which online kernels can take it."""
    if d <= 4:
        return "registers"          # k_seq_r / k_scan stages for itself
    if d <= 8:
        return "staged"             # k_scan over LDS-staged rows
    if d <= WINDOW_MAX_DIM:
        from chronoclust_amd import _lib
        return "ladder" if _lib.scan_width(d, False, True)[0] == d else "padded"
    return "hbm" if d <= 128 else "wide"


# ---- 2. whole streams on a lived handle -------------------------------------------------------------------------------------

# (kind, seed): test_fuzz_parity._case, test_sequential._seq_r_case, a stream of test_any_dims' kind at d = 129.  Widths in
# this order: 2 1 64 129 33 2 3 4 17 9 4 64 17 - forwards and reversed every width but the ends of the range has a wider and
# a narrower predecessor; k = 0.5, 1, 2, 3, 4, 40, pi below d and not, lambda 0 .. 5, windows of 1, 5, 64, 700, 1 024 and
# 4 096 points, tables of a handful to 4 000 rows all occur.
STREAMS = [("seq_r", 42), ("fuzz", 67), ("fuzz", 17), ("wide", 129), ("fuzz", 119), ("fuzz", 79), ("seq_r", 27), ("seq_r", 37),
           ("fuzz", 134), ("fuzz", 28), ("fuzz", 157), ("fuzz", 61), ("fuzz", 45)]
ORDERS = {"forwards": STREAMS, "reversed": STREAMS[::-1]}
RESTORED = ("fuzz", 119)     # its state is taken when it finishes and restored at the end of the life, into another width
LOOKAHEADS = (3, 0, 2)


def wide_stream(d, n=1500, seed=0):
    """A stream of tests/test_any_dims.py's kind: anisotropic blobs, 2 % uniform noise, decay and deletion, populations
    that end."""
    import scenarios
    rng = np.random.default_rng(10240 + seed)
    g = int(rng.integers(4, 30))
    sigma = float(rng.choice([0.004, 0.015, 0.03]))
    k, pi = 3.0, d - 3
    wide = np.zeros((g, d), dtype=bool)
    for i in range(g):
        wide[i, rng.choice(d, int(rng.integers(4, 9)), replace=False)] = True
    sig = np.where(wide, 0.08, sigma)
    eps = float(np.sqrt(0.8 * (d * sigma * sigma / k + 6 * 0.0064)))
    cfg = scenarios.params_to_config(scenarios.blob_params(n, param_epsilon=eps, param_k=k, param_pi=pi, param_lambda=0.5,
                                                            param_omicron=0.0003, promote_after=3))
    centres = rng.uniform(0.1, 0.9, (g, d))
    Xs = []
    for t in range(3):
        lab = rng.integers(0, g, n)
        X = np.clip(centres[lab] + rng.normal(0.0, 1.0, (n, d)) * sig[lab], 0.0, 1.0)
        noise = rng.random(n) < 0.02
        X[noise] = rng.random((int(noise.sum()), d))
        Xs.append(np.ascontiguousarray(X))
        centres = np.clip(centres + rng.normal(0.0, 0.004, centres.shape), 0.0, 1.0)
        if t == 0:
            centres, sig, g = centres[: max(1, g - 2)], sig[: max(1, g - 2)], max(1, g - 2)
    return cfg, Xs


_streams = {}


def stream(key):
    """(config, window, timepoints) of a stream."""
    if key not in _streams:
        kind, seed = key
        if kind == "fuzz":
            from test_fuzz_parity import _case
            cfg, window, Xs = _case(seed)
        elif kind == "seq_r":
            from test_sequential import _seq_r_case
            cfg, Xs = _seq_r_case(seed)
            window = 1024
        else:
            cfg, Xs = wide_stream(seed)
            window = 1024
        _streams[key] = (cfg, window, Xs)
    return _streams[key]


def stream_dim(key):
    return stream(key)[2][0].shape[1]


class Snapshot(object):
    """What _check_against_oracle reads of an oracle, kept after the oracle has moved on."""

    def __init__(self, o):
        self.labels_uid, self.paths, self.counters = o.labels_uid.copy(), o.paths.copy(), o.counters
        self._tables = {kind: o.table(kind) for kind in (0, 1)}
        self.clusters = o.clusters

    def table(self, kind):
        return self._tables[kind]


class ListsSnapshot(object):
    """Both lists and the counters of an oracle at one moment, in the shape table_util.same_lists reads."""

    def __init__(self, o):
        self._tables = {kind: o.table(kind) for kind in (0, 1)}
        self.counters = o.counters

    def table(self, kind):
        return self._tables[kind]

    def rows(self):
        return len(self._tables[0]["id"]) + len(self._tables[1]["id"])


_snapshots = {}


def continuation(key):
    """The timepoint a restored stream continues with (daystamp = its number of timepoints)."""
    Xs = stream(key)[2]
    return np.ascontiguousarray(Xs[0][::2] * 0.5 + 0.25), len(Xs)


def stream_oracle(key):
    """The oracle's state after every timepoint of a stream - and, for RESTORED, after its continuation."""
    if key not in _snapshots:
        from oracle import oracle as O
        cfg, _, Xs = stream(key)
        o = O.OracleHDDStream(cfg)
        snaps = []
        for t, X in enumerate(Xs):
            o.online_microcluster_maintenance(X, t)
            snaps.append(Snapshot(o))
        if key == RESTORED:
            X, day = continuation(key)
            o.online_microcluster_maintenance(X, day)
            snaps.append(Snapshot(o))
        _snapshots[key] = snaps
    return _snapshots[key]


def adopt(handle, cfg):
    """An HDDStream that runs on `handle` instead of the one it made."""
    from chronoclust_amd.clustering.hddstream import HDDStream
    s = HDDStream(cfg)
    s._h.close()
    s._h = handle
    return s


def stream_tuning(mode, key, position):
    return dict(MODES[mode][1], window=stream(key)[1], lookahead=LOOKAHEADS[position % 3])


def check_stream_regime(mode, key, X, s):
    n, d = X.shape
    assert s["points"] == n, s
    if d > WINDOW_MAX_DIM:
        assert s["seq_g_points"] == n and s["windows"] == 0, s
    elif MODES[mode][1].get("sequential") == 1:
        assert s["windows"] > 0 and s["seq_points"] == 0 and s["seq_g_points"] == 0, s


def run_stream(handle, mode, key, position, take_state=False):
    """A whole stream on `handle` (reset first), the oracle after every timepoint; returns get_state() of the finished stream
    where asked."""
    from test_hip_parity import _check_against_oracle
    cfg, _, Xs = stream(key)
    snaps = stream_oracle(key)
    s = adopt(handle, cfg)
    handle.reset()
    handle.set_tuning(**stream_tuning(mode, key, position))
    for t, X in enumerate(Xs):
        s.online_microcluster_maintenance(X, t)
        _check_against_oracle(s, snaps[t])
        check_stream_regime(mode, key, X, handle.stats())
    return s.get_state() if take_state else None


def run_restored(handle, mode, state):
    """set_state of RESTORED's finished stream into `handle` - which has since run streams of other widths -, one more
    timepoint, the oracle continued likewise."""
    from test_hip_parity import _check_against_oracle
    cfg = stream(RESTORED)[0]
    X, day = continuation(RESTORED)
    s = adopt(handle, cfg)
    s.set_state(state)
    handle.set_tuning(**stream_tuning(mode, RESTORED, 0))
    s.online_microcluster_maintenance(X, day)
    _check_against_oracle(s, stream_oracle(RESTORED)[-1])
    check_stream_regime(mode, RESTORED, X, handle.stats())


def run_stream_life(order, mode):
    keys = ORDERS[order]
    h = new_handle(mode)
    state = None
    try:
        for pos, key in enumerate(keys):
            def fresh(pos=pos, key=key):
                f = new_handle(mode)
                try:
                    run_stream(f, mode, key, pos)
                finally:
                    f.close()

            def lived(pos=pos, key=key):
                return run_stream(h, mode, key, pos, take_state=key == RESTORED)
            box = []
            located(lambda: box.append(lived()), fresh, "streams %s[%s] %d %r" % (order, mode, pos, key))
            if key == RESTORED:
                state = box[0]
        assert stream_dim(keys[-1]) != stream_dim(RESTORED)

        def fresh_restore():
            f = new_handle(mode)
            try:
                run_restored(f, mode, state)
            finally:
                f.close()
        located(lambda: run_restored(h, mode, state), fresh_restore, "streams %s[%s] restore of %r" % (order, mode, RESTORED))
    finally:
        h.close()


# ---- 3. lives without reset() -----------------------------------------------------------------------------------------------

def oracle_point_clusters(labels_uid, pcore_table, clusters):
    """cc_point_clusters as the oracle's results imply it: the numpy join of chronoclust_amd.multi over the oracle's labels,
    pcore list and clusters."""
    from chronoclust_amd import multi
    mem = np.concatenate([np.asarray(c["members"], np.int64) for c in clusters]) if clusters else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum([len(c["members"]) for c in clusters])]).astype(np.int64)
    return multi.point_cluster_index(labels_uid, pcore_table["id"], pcore_table["uid"], mem, off)


EMPTIED_FIRST, EMPTIED_THEN = "clean-60+30x20", "clean-100+50x13"
EMPTIED_FACTOR = 2.0 ** -10
_emptied = {}


def emptied():
    """The oracle's side of "a table that decay empties, then another width": EMPTIED_FIRST's table and points at d = 20, its
    offline phase, cc_decay_downgrade with 2^-10 until both lists are empty (the reference removes from the lists it iterates
    over, so one call never deletes all: `decays` holds the lists after each call), then EMPTIED_THEN's points - no table -
    at d = 13 in a new oracle that continues the id counters."""
    if not _emptied:
        from oracle import oracle as O
        c = build(EMPTIED_FIRST)
        o = T.make_oracle(c[2], c[0], c[1])
        o.online_microcluster_maintenance(c[3], 0, reset_param=False, offline=False)
        first = dict(o=ListsSnapshot(o), uid=o.labels_uid.copy(), path=o.paths.copy(), tables=[o.table(0), o.table(1)], counters=o.counters,
                     offline=T.oracle_offline(o))
        decays = []
        while len(o.table(0)["id"]) + len(o.table(1)["id"]) and len(decays) < 64:
            O.lib().co_decay_downgrade(o._h, EMPTIED_FACTOR)
            decays.append(ListsSnapshot(o))
        c2 = build(EMPTIED_THEN)
        o2 = T.make_oracle(c2[2])
        o2.set_counters(*o.counters)
        o2.online_microcluster_maintenance(c2[3], 0, reset_param=False, offline=False)
        then = dict(o=o2, uid=o2.labels_uid.copy(), path=o2.paths.copy())
        off = T.oracle_offline(o2)
        _emptied.update(first_case=c, first=first, old=o, decays=decays, then_case=c2, then=then, then_offline=off,
                        then_point_clusters=oracle_point_clusters(then["uid"], o2.table(0), off[1]))
    return _emptied


# timepoint sizes of the prefetch life; at d = 16 every timepoint (float32) is prefetched and adopted, at d = 20 a decoy of the same shape
# is prefetched and the upload of the real array discards it
PREFETCH_SIZES = (20000, 1, 3000, 64, 20000)
_prefetch = {}


def prefetch_stream(d):
    """(config, timepoints, decoys, the oracle's snapshots, its pcore centroids per timepoint)."""
    if d not in _prefetch:
        import scenarios
        from oracle import oracle as O
        cfg = scenarios.params_to_config(scenarios.blob_params(PREFETCH_SIZES[0], param_omicron=0.0002, param_lambda=1.0))
        Xs = [scenarios.make_blobs(500 + d, n, d, 60) for n in PREFETCH_SIZES]
        if d == 16:                                              # float32 as it lies: cc_f32_points counts what the handle took
            Xs = [np.ascontiguousarray(X.astype(np.float32)) for X in Xs]
        decoys = [scenarios.make_blobs(900 + d + t, n, d, 7) for t, n in enumerate(PREFETCH_SIZES)]
        o = O.OracleHDDStream(cfg)
        snaps = []
        for t, X in enumerate(Xs):
            o.online_microcluster_maintenance(X, t)
            snaps.append(Snapshot(o))
        _prefetch[d] = (cfg, Xs, decoys, snaps)
    return _prefetch[d]


# collapse and regrowth: 30 000 populations, 16 000 points - about 12 000 microclusters from an empty table in one call -, three
# decays by 1/4 (pcores below beta mu = 2 are downgraded, outliers up to omicron = 1 deleted), 500 points, 12 000 points
COLLAPSE = dict(seed=77, d=20, g=30000, sizes=(16000, 500, 12000), factor=0.25, decays=3)
COLLAPSE_PAR = T.Params(0.05 ** 2, 0.05 ** 2, 4.0, 0.5, 4.0, 1.0, 0.5, 0.25, 0.05, 20)
_collapse = {}


def collapse():
    """The oracle's side: per online call (uid, path, lists, counters); the offline phase after the 500-point call."""
    if not _collapse:
        import scenarios
        from oracle import oracle as O
        sc = COLLAPSE
        Xs = [scenarios.make_blobs(sc["seed"], n, sc["d"], sc["g"]) for n in sc["sizes"]]
        o = T.make_oracle(COLLAPSE_PAR)
        calls, rows = [], []
        for t, X in enumerate(Xs):
            if t == 1:
                for _ in range(sc["decays"]):
                    O.lib().co_decay_downgrade(o._h, sc["factor"])
                rows.append(len(o.table(0)["id"]) + len(o.table(1)["id"]))
            o.online_microcluster_maintenance(X, 0, reset_param=False, offline=False)
            calls.append(dict(o=ListsSnapshot(o), uid=o.labels_uid.copy(), path=o.paths.copy()))
            rows.append(calls[-1]["o"].rows())
            if t == 1:
                off = T.oracle_offline(o)
        _collapse.update(Xs=Xs, calls=calls, rows=rows, offline=off)   # rows: after call 0, after the decays, after calls 1, 2
    return _collapse


# ---- 4. read-only calls -----------------------------------------------------------------------------------------------------

READONLY = {"clean-300+150x13": 300, "clean-2000+1000x20": 2048}
HIGH_COUNTERS = (3_000_000, 3_000_000)   # above every injected creation number: cc_point_clusters maps creation numbers below the counter
_readonly = {}


def readonly(name):
    """The oracle's side of the read-only life of a table case cut to READONLY[name] points: the run's result, its offline phase
    and point clusters; the queries the interposed calls ask."""
    if name not in _readonly:
        c = build(name)
        X = np.ascontiguousarray(c[3][:READONLY[name]])
        assert len(X) == READONLY[name]
        o = T.make_oracle(c[2], c[0], c[1])
        o.set_counters(*HIGH_COUNTERS)
        before = T.oracle_offline(T.make_oracle(c[2], c[0], c[1]))
        o.online_microcluster_maintenance(X, 0, reset_param=False, offline=False)
        exp = dict(o=o, uid=o.labels_uid.copy(), path=o.paths.copy())
        off = T.oracle_offline(o)
        rng = np.random.default_rng(len(name))
        d = X.shape[1]
        Q = np.ascontiguousarray(np.concatenate([X[::3] + rng.normal(0.0, 0.002, X[::3].shape), rng.uniform(0.1, 0.9, (64, d))]))
        _readonly[name] = dict(case=c, X=X, exp=exp, offline_before=before, offline=off, Q=Q,
                               point_clusters=oracle_point_clusters(exp["uid"], o.table(0), off[1]))
    return _readonly[name]


def sources(Q):
    """The four kinds of source of the values Q: float64 rows, float32 rows, a view (Fortran order, float64) and list-mode
    records (float32, big-endian, one byte past an aligned address)."""
    import transform_util as U
    f32 = np.ascontiguousarray(Q.astype(np.float32))
    return {"f64": np.ascontiguousarray(Q), "f32": f32, "view": np.asfortranarray(Q), "list": U.list_mode(f32, U.BIG)}
