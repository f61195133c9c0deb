"""Widths that are not one of the compiled ones (9 <= d <= 64 off the ladder 14 / 16 / 20 / 32 / 40 / 64) on the
scalar-operand scan and the pruned chain: the kernels run at the next compiled width over padded operands - the points'
dimension-major copy with zero rows behind the d real ones, the rows' centroids and operands from the mirror k_pad_rows
rebuilds in front of every snapshot scan.  A padded dimension adds (0 - 0)^2 * 1 = +0 to a sum of
non-negative terms, so every result must be the oracle's bit for bit, as at the compiled widths.  Modelled on
tests/test_pruned_scan.py; the knobs are read when a handle is created, so each case sets them around the constructor."""
import numpy as np
import pytest

import scenarios
from test_pruned_scan import _against_oracle, _env, _hdd, _same_state

pytestmark = pytest.mark.gpu

COUNTERS = ("scan_u_launches", "scan_p_launches", "scan_g_launches", "pad_rows_launches", "missed_points", "windows")


def _add(tot, s):
    for k in COUNTERS:
        tot[k] = tot.get(k, 0) + s[k]
    return tot


def _run_against_oracle(h, cfg, Xs):
    """Every timepoint against the oracle; the counters summed over the calls."""
    from oracle import oracle as O
    o = O.OracleHDDStream(cfg)
    tot = {}
    for t, X in enumerate(Xs):
        h.online_microcluster_maintenance(X, t)
        o.online_microcluster_maintenance(X, t)
        _against_oracle(h, o)
        _add(tot, h.stats())
    assert tot["windows"] > 0, tot  # the windowed path ran
    return tot, o


FORCED = [
    # (seed, n, d, g, sigma, parameter overrides, tuning, shift): the shapes of test_pruned_scan.CASES at the neighbouring width
    (41, 6000, 9, 120, 0.01, {}, dict(window=1024), 0.0),    # one real dimension beyond the eight of the prefix, five padded
    (42, 6000, 13, 120, 0.01, {}, dict(window=1024), 0.0),   # one padded dimension
    (43, 5000, 15, 60, 0.02, dict(param_k=8), dict(window=512, lookahead=2), 0.0),
    (44, 9000, 18, 300, 0.01, {}, dict(window=2048), 0.0),
    (45, 5000, 21, 60, 0.01, dict(param_k=2), dict(window=1024), 0.0),  # eleven padded, three inside the second MFMA's 8 .. 23
    (46, 6000, 37, 150, 0.01, {}, dict(window=4096), 0.0),
    (47, 4000, 41, 30, 0.01, {}, dict(window=1024), 0.0),    # 23 padded at 64: k_scan_p's form, the high mask word
    (48, 4000, 63, 30, 0.01, {}, dict(window=1024), 0.0),    # one padded at 64
    # d = 18: k < 1 (a preferred dimension weighs more), coordinates around 1 000, heavy overlap (nearly every row completed)
    (49, 6000, 18, 100, 0.01, dict(param_k=0.5), dict(window=1024), 0.0),
    (50, 6000, 18, 200, 0.01, {}, dict(window=2048), 1000.0),
    (51, 5000, 18, 12, 0.15, dict(param_epsilon=0.2), dict(window=512), 0.0),
]


@pytest.mark.parametrize("seed,n,d,g,sigma,over,tuning,shift", FORCED)
def test_forced_pruning_matches_the_oracle(seed, n, d, g, sigma, over, tuning, shift):
    cfg = scenarios.params_to_config(scenarios.blob_params(n, **over))
    h = _hdd(cfg, 2, **tuning)
    Xs = [scenarios.make_blobs(seed * 100 + t, n, d, g, sigma) + shift for t in range(3)]
    tot, _ = _run_against_oracle(h, cfg, Xs)
    assert tot["scan_p_launches"] > 0 and tot["scan_u_launches"] > 0, tot
    assert tot["pad_rows_launches"] > 0, tot


@pytest.mark.parametrize("lookahead", [3, 2])
@pytest.mark.parametrize("seed,n,d,g,window", [(61, 6000, 18, 120, 1024), (62, 4000, 41, 30, 512)])
def test_plain_scans_with_lookahead(seed, n, d, g, window, lookahead):
    """k_scan_u alone, the lookahead scans on the second stream: the mirrors of both window parities."""
    cfg = scenarios.params_to_config(scenarios.blob_params(n))
    h = _hdd(cfg, 0, window=window, lookahead=lookahead)
    Xs = [scenarios.make_blobs(seed * 100 + t, n, d, g, 0.01) for t in range(3)]
    tot, _ = _run_against_oracle(h, cfg, Xs)
    assert tot["scan_u_launches"] > 0 and tot["scan_p_launches"] == 0, tot
    assert tot["pad_rows_launches"] > 0, tot


def test_default_policy_uses_the_pruned_chain_in_the_steady_state():
    """The shape of test_pruned_scan's default-policy case at 18 dimensions, against a handle that never prunes."""
    n, d, g = 400_000, 18, 2000
    X = scenarios.make_blobs(5, n, d, g)
    cfg = scenarios.params_to_config(scenarios.blob_params(n))
    auto, plain = _hdd(cfg, 1), _hdd(cfg, 0)
    auto.online_microcluster_maintenance(X, 0)
    plain.online_microcluster_maintenance(X, 0)
    _same_state(auto, plain)
    s = auto.stats()
    assert s["windows"] > 0
    assert 0 < s["scan_p_launches"] < s["scan_u_launches"], s
    assert s["scan_g_launches"] > 0, s
    assert plain.stats()["scan_p_launches"] == 0 and plain.stats()["scan_u_launches"] > 0


def test_guessed_thresholds_miss_a_loose_population():
    """The stream of test_pruned_scan's case of this name, cut to 18 columns: the missed points go through k_missed and
    the plain scan over their list (k_scan_u with a point list) on padded operands."""
    rng = np.random.default_rng(31)
    n, d, g = 60_000, 20, 300
    centres = rng.uniform(0.1, 0.9, (g, d))
    sig = np.where(np.arange(g) < 240, 0.004, 0.03)
    cfg = scenarios.params_to_config(scenarios.blob_params(n, param_epsilon=0.25))
    guess = _hdd(cfg, 2, window=8192)
    Xs = []
    for t in range(3):
        lab = rng.integers(0, g, n)
        X = np.clip(centres[lab] + rng.normal(0.0, 1.0, (n, d)) * sig[lab, None], 0.0, 1.0)
        Xs.append(np.ascontiguousarray(X[:, :18]))
    tot, _ = _run_against_oracle(guess, cfg, Xs)
    print("guessed-threshold launches %d, points missed %d" % (tot["scan_g_launches"], tot["missed_points"]))
    assert tot["missed_points"] > 0 and tot["scan_g_launches"] > 0, tot
    assert tot["pad_rows_launches"] > 0


EXTREME = [
    ("2^130", 2.0 ** 130, None),                      # coordinates overflow single precision: inf - inf in the prefix
    ("one huge late column", 1.0, (17, 2.0 ** 130)),  # ... in the last real dimension, next to the padded ones
]


@pytest.mark.parametrize("name,scale,column", EXTREME, ids=[e[0] for e in EXTREME])
@pytest.mark.parametrize("prune", [2, 1])
def test_coordinates_outside_single_precision_range(name, scale, column, prune):
    n, d, g = 5000, 18, 80
    eps = 0.05 * scale * (column[1] if column else 1.0)
    cfg = scenarios.params_to_config(scenarios.blob_params(n, param_epsilon=eps))
    h = _hdd(cfg, prune, window=1024)
    Xs = []
    for t in range(2):
        X = scenarios.make_blobs(900 + t, n, d, g) * scale  # (a power of two: exact)
        if column:
            X[:, column[0]] *= column[1]
        assert np.isfinite(X).all()
        Xs.append(X)
    tot, _ = _run_against_oracle(h, cfg, Xs)
    assert tot["pad_rows_launches"] > 0 and tot["scan_u_launches"] > 0, tot
    if prune == 2:
        assert tot["scan_p_launches"] > 0, tot


@pytest.mark.parametrize("scale,k,all_dims", [(1e-154, 4.0, False), (1e-158, 2.0, False), (1e-200, 4.0, False),
                                              (3e-121, 16.0, False), (1e-153, 4.0, True), (2e-154, 2.0, True)])
def test_subnormal_distance_terms(scale, k, all_dims):
    """test_hip_parity's case of this name at 18 dimensions: a wave or a tile that holds a nonzero coordinate below 2^-400
    takes the unfused loop.  The padded zeros are not tiny - they must not send a wave there - and a padded term is +0 in
    either loop - they need not.  (sequential=1: twelve microclusters would go to the sequential kernel.)"""
    n, d, g = 3000, 18, 12
    cfg = scenarios.params_to_config(scenarios.blob_params(n, param_k=k, param_epsilon=0.06 * (scale if all_dims else 1.0),
                                                           param_delta=0.05 * (scale if all_dims else 1.0)))
    h = _hdd(cfg, 1, window=512, lookahead=3, sequential=1)
    Xs = []
    for t in range(2):
        X = scenarios.make_blobs(4100 + t, n, d, g, 0.02)
        if all_dims:
            X *= scale
        else:
            X[:, 1] *= scale
            X[:, 4] *= scale * 7.0
            X[:, 17] *= scale * 3.0  # (the last real dimension)
        X[::5, 2] = 0.0
        Xs.append(X)
    tot, _ = _run_against_oracle(h, cfg, Xs)
    assert tot["scan_u_launches"] > 0 and tot["pad_rows_launches"] > 0, tot


@pytest.mark.parametrize("wps", [1, 3])
def test_table_growth_across_the_mirror_capacity(wps):
    """test_hip_parity's lookahead-and-growth stream at 18 dimensions: rows are created in every window, the table outgrows
    its allocation several times, and the mirror has to follow it (between batches, both parities)."""
    n, d, g = 7000, 18, 10
    cfg = scenarios.params_to_config(scenarios.blob_params(n, param_epsilon=0.05))
    h = _hdd(cfg, 1, window=64, windows_per_sync=wps, lookahead=3, sequential=1)
    Xs = [scenarios.make_blobs(800 + t, n, d, g, 0.2) for t in range(2)]
    tot, o = _run_against_oracle(h, cfg, Xs)
    assert len(o.table(1)["id"]) + len(o.table(0)["id"]) > 1100  # the table was reallocated at least once
    assert tot["scan_u_launches"] > 0 and tot["pad_rows_launches"] > 0, tot


def _any_width_case(seed):
    """_fuzz_case of tests/test_pruned_scan.py (the same draws in the same order) with d drawn from widths off the ladder,
    the columns generated at that width."""
    rng = np.random.default_rng(7000 + seed)
    d = int(rng.choice([9, 13, 18, 25, 30, 37, 50, 63]))
    n = int(rng.choice([1, 17, 300, 1500, 4000]))
    g = int(rng.choice([1, 2, 5, 12, 40, 150]))
    sigma = float(rng.choice([0.0, 0.001, 0.02, 0.08, 0.3]))
    grid = bool(rng.random() < 0.3)
    cfg = {
        "beta": float(rng.choice([0.1, 0.5, 0.9, 1.0])),
        "delta": float(rng.choice([0.0, 0.01, 0.05, 0.3, 1.0])),
        "epsilon": float(rng.choice([0.001, 0.03, 0.1, 0.5, 3.0])),
        "lambda": float(rng.choice([0.0, 0.5, 2.0, 5.0])),
        "k": float(rng.choice([0.5, 1.0, 2.0, 4.0, 16.0])),
        "mu": float(rng.choice([0.0005, 0.002, 0.01, 0.1])),
        "pi": int(rng.choice([0, d, d + 3])),
        "omicron": float(rng.choice([0.0, 1e-5, 1e-3, 0.05])),
        "upsilon": float(rng.choice([0.5, 1.0, 3.0, 6.5, 20.0])),
    }
    window = int(rng.choice([5, 64, 700, 4096]))
    lookahead = int(rng.choice([0, 2, 3]))
    F = float(rng.choice([1.0, 2.0, 16.0, 16.0, 1024.0]))
    shift = float(rng.choice([0.0, 0.0, 100.0, -3.0e4]))
    centres = rng.uniform(0.1, 0.9, (g, d))
    Xs = []
    for t in range(3):
        nt = max(1, int(n * rng.choice([1.0, 0.5, 0.1]))) if t else n
        lab = rng.integers(0, g, nt)
        X = np.clip(centres[lab] + rng.normal(0.0, 1.0, (nt, d)) * sigma, 0.0, 1.0)
        if grid:
            X = np.round(X * 8) / 8
        Xs.append(np.ascontiguousarray(X + shift))
        centres = np.clip(centres + rng.normal(0, 0.02, centres.shape), 0, 1)
    return cfg, window, lookahead, F, Xs


@pytest.mark.parametrize("seed", range(48))
def test_forced_pruning_fuzz(seed):
    """(sequential=1: the small tables of these streams would go to the sequential kernels, and no scan would run.)"""
    cfg, window, lookahead, F, Xs = _any_width_case(seed)
    h = _hdd(cfg, 2, F=F, window=window, lookahead=lookahead, sequential=1)
    tot, _ = _run_against_oracle(h, cfg, Xs)
    assert tot["scan_u_launches"] > 0 and tot["pad_rows_launches"] > 0, tot
    assert tot["scan_p_launches"] > 0, tot


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 3])
def test_scan_split_over_the_ranks_of_a_group(world):
    """In-process ranks with every split forced on from the first window (thresholds 0), pruning forced: each rank pads all
    rows (the seeds go over the whole table on every rank) and scans its share; bit-equal to one handle."""
    import pipeline_util as PU
    from test_sharded_local import run_group
    sc = dict(seed=19, n=12_000, d=18, g=300, sigma=0.01, timepoints=3, drift=0.01, churn=0.08)
    cfg = scenarios.params_to_config(scenarios.blob_params(sc["n"], param_omicron=0.0002, param_lambda=2))
    Xs = scenarios.make_blob_timepoints(sc, raw=True)
    tuning = dict(window=2048, lookahead=3)
    single = PU.run_pipeline(Xs, cfg, tuning=tuning)
    for env in (dict(CHRONOCLUST_HIP_PRUNE=2), dict(CHRONOCLUST_HIP_PRUNE=0)):
        for res in run_group(world, Xs, cfg, tuning=tuning, env=env):
            PU.same_results(res, single)
            st = [r["stats"] for r in res]
            assert sum(s["sharded_windows"] for s in st) > 0 and sum(s["pad_rows_launches"] for s in st) > 0
            assert sum(s["scan_u_launches"] for s in st) > 0
            assert (sum(s["scan_p_launches"] for s in st) > 0) == (env["CHRONOCLUST_HIP_PRUNE"] == 2)


@pytest.mark.parametrize("seed,n,d,g,tuning", [(21, 9000, 20, 300, dict(window=2048)),
                                                (22, 9000, 14, 120, dict(window=1024, lookahead=3))])
def test_unchanged_at_the_ladder(seed, n, d, g, tuning):
    """d == the compiled width: the same kernels as ever, straight on the table - no pad pass."""
    cfg = scenarios.params_to_config(scenarios.blob_params(n))
    h = _hdd(cfg, 2, **tuning)
    Xs = [scenarios.make_blobs(seed * 100 + t, n, d, g, 0.01) for t in range(3)]
    tot, _ = _run_against_oracle(h, cfg, Xs)
    assert tot["scan_p_launches"] > 0 and tot["scan_u_launches"] > 0, tot
    assert tot["pad_rows_launches"] == 0, tot
