"""k_decide with 16-lane groups (d <= 32) and 32-lane groups (beyond, or CHRONOCLUST_HIP_DECIDE_GROUP=32), and the window's
displacement maxima of k_dseed with its loads in flight.

What can go wrong with a narrower group: a lane that owns the wrong dimension (d around 16 and 32: one / two dimensions per
lane, the last 16-lane and the first 32-lane width), a ballot that is not sliced to the group's bits (the pdim filter decides
on it), groups of one wave that go different ways through the decision procedure (creation, promotion, deletion, refused
points: three timepoints with decay), a wave that is only partly filled (odd windows), the carry workgroups at the end of a
grid whose size k_decide now derives itself (lookahead), the atomics of the claims (CHRONOCLUST_HIP_CLAIMS=0) and the merge of
gathered records inside a row of 16 lanes (an in-process group of two ranks).  Every case is compared with the CPU oracle after
every timepoint, and at d <= 32 the two widths referee each other byte for byte.

k_dseed reads (B + 15) / 16 records of the window's tile maxima, eight per lane and trip: window sizes whose record count is no
multiple of 64 nor of 512, with lookahead (the carry set's column) off and on, on a settled table so that every window has the
size that is asked for."""
import numpy as np
import pytest

import pipeline_util as P
import scenarios
import test_fuzz_parity as F
import test_hip_parity as H
import test_pruned_scan as PS
import test_sharded_local as SL

pytestmark = pytest.mark.gpu

WIDE = dict(CHRONOCLUST_HIP_DECIDE_GROUP=32)  # one 32-lane group per point whatever d


def _stream(d, n=4000, seed=0, **over):
    """Three timepoints with decay (lambda = 2, omicron > 0): population A; half A, half B; B alone - microclusters are
    created, promoted (A, then B), decay, are downgraded and deleted.  In one or two dimensions only a few blobs fit side by
    side."""
    g = {1: 4, 2: 8}.get(d, 60)
    cfg = scenarios.params_to_config(scenarios.blob_params(n, param_omicron=0.0002, param_lambda=2, **over))
    a, b = 1000 + 10 * d + seed, 2000 + 10 * d + seed
    rng = np.random.default_rng(a)
    mix = np.vstack([scenarios.make_blobs(a, n // 2 + 1, d, g), scenarios.make_blobs(b, n // 2, d, g)])
    Xs = [scenarios.make_blobs(a, n, d, g), mix, scenarios.make_blobs(b, n - 7, d, g)]
    # ... and thirty stray points per timepoint: outlier microclusters of weight 1 that the next boundary deletes
    Xs = [np.vstack([X, rng.uniform(0.0, 1.0, (30, d))]) for X in Xs]
    return cfg, [np.ascontiguousarray(X[rng.permutation(len(X))]) for X in Xs]


def _run(cfg, Xs, env=None, oracle=True, **tuning):
    """The stream through a handle created under `env`, compared with the oracle after every timepoint; returns the handles'
    states per timepoint (labels, paths, id counters, both tables) for the cross-check of the widths."""
    from oracle import oracle as O
    with P.knobs(**(env or {})):
        h = H._hdd(cfg, **tuning)
    o = O.OracleHDDStream(cfg) if oracle else None
    states = []
    for t, X in enumerate(Xs):
        h.online_microcluster_maintenance(X, t)
        if o is not None:
            o.online_microcluster_maintenance(X, t)
            H._check_against_oracle(h, o)
        states.append((h.labels_uid.copy(), h.labels_path.copy(), (h.pcore_MC_last_id, h.outlier_MC_last_id),
                       [{k: np.array(v) for k, v in h.table(kind).items()} for kind in (0, 1)]))
    return states, o


def _same_states(a, b):
    for (la, pa, ca, ta), (lb, pb, cb, tb) in zip(a, b):
        assert la.tobytes() == lb.tobytes() and pa.tobytes() == pb.tobytes() and ca == cb
        for x, y in zip(ta, tb):
            for key in ("id", "uid", "w", "cf1", "cf2", "cen", "pref"):
                assert x[key].shape == y[key].shape and x[key].tobytes() == y[key].tobytes(), key


DIMS = [1, 2, 15, 16, 17, 20, 31, 32, 33, 40]


@pytest.mark.parametrize("d", DIMS)
def test_dimensionality(d):
    cfg, Xs = _stream(d)
    states, o = _run(cfg, Xs, window=1024, lookahead=3 if d % 2 else 2)
    # the stream does what it is built for (conditions on the oracle's own output)
    paths = set(int(x) for x in np.unique(np.concatenate([s[1] for s in states])))
    assert {0, 1, 2} <= paths, paths  # joined a pcore microcluster, an outlier microcluster, created one
    assert len(o.table(0)["id"]) > 0  # promoted
    if d >= 15:  # (in one or two dimensions the stray points fall into the blobs)
        assert o.counters[1] > len(o.table(0)["id"]) + len(o.table(1)["id"])  # more created than are left: deleted


@pytest.mark.parametrize("d", [x for x in DIMS if x <= 32])
def test_widths_agree(d):
    """The same streams once more with 32-lane groups: the default run's labels, tables and id counters byte for byte."""
    cfg, Xs = _stream(d)
    tuning = dict(window=1024, lookahead=3 if d % 2 else 2)
    narrow, _ = _run(cfg, Xs, oracle=False, **tuning)
    wide, _ = _run(cfg, Xs, env=WIDE, **tuning)
    _same_states(narrow, wide)


@pytest.mark.parametrize("window", [1, 2, 3, 5, 63, 65, 1025])
def test_partly_filled_waves(window):
    """Windows that leave a wave of k_decide partly filled (four points per wave at 16 lanes, sixteen per workgroup)."""
    cfg, Xs = _stream(20, n=200 if window <= 5 else 3000)
    _run(cfg, Xs, window=window)


def _filter_stream(d, n=4000, g=40):
    """Blobs with 0 - 3 wide dimensions (the first ones, by blob number): d - wide preferred dimensions against pi = d - 2, so
    the count behind the ballots passes for half of the blobs and fails for the others."""
    cfg = scenarios.params_to_config(scenarios.blob_params(n, param_pi=d - 2, param_epsilon=0.25, param_omicron=0.0002, param_lambda=2))
    Xs = []
    for t in range(3):
        rng = np.random.default_rng(500 + d)  # (the same blobs in every timepoint)
        centres = rng.uniform(0.1, 0.9, (g, d))
        rng = np.random.default_rng(600 + 10 * d + t)
        lab = rng.integers(0, g, n - 3 * t)
        X = centres[lab] + rng.normal(0.0, 0.01, (len(lab), d))
        wide = (np.arange(d)[None, :] < (lab % 4)[:, None])
        X = X + wide * rng.normal(0.0, 0.08, X.shape)
        Xs.append(np.ascontiguousarray(np.clip(X, 0.0, 1.0)))
    return cfg, Xs


REGIMES = {
    "pdim filter": None,
    "k 3": (dict(param_k=3), {}, {}),
    "lookahead": ({}, {}, dict(lookahead=3)),  # (the cc_apply_carry workgroups at the end of k_decide's round-0 grid)
    "claims by atomics": ({}, dict(CHRONOCLUST_HIP_CLAIMS=0), {}),
}


@pytest.mark.parametrize("d", [20, 32])
@pytest.mark.parametrize("regime", sorted(REGIMES), ids=lambda r: r.replace(" ", "_"))
def test_decision_regimes(regime, d):
    if regime == "pdim filter":
        cfg, Xs = _filter_stream(d)
        states, o = _run(cfg, Xs, window=1024)
        assert {0, 1, 2} <= set(int(x) for x in np.unique(np.concatenate([s[1] for s in states])))
        assert len(o.table(0)["id"]) > 0 and len(o.table(1)["id"]) > 0  # some blobs pass the filter, some never do
        return
    over, env, tuning = REGIMES[regime]
    cfg, Xs = _stream(d, seed=3, **over)
    _run(cfg, Xs, env=env, **dict(dict(window=1024), **tuning))


@pytest.mark.parametrize("d", [20, 32])
def test_group_of_two_ranks(d):
    """Round 0 reads the gathered records (one merged record per rank and point, part_inner = 1): the one-GPU results on both
    ranks."""
    sc = dict(seed=9 + d, n=4000, d=d, g=150, sigma=0.01, timepoints=3, drift=0.01, churn=0.08)
    cfg = scenarios.params_to_config(scenarios.blob_params(sc["n"], param_omicron=0.0002, param_lambda=2))
    Xs = scenarios.make_blob_timepoints(sc, raw=True)
    single = P.run_pipeline(Xs, cfg)
    for res in SL.run_group(2, Xs, cfg, tuning=dict(window=1024, lookahead=3)):
        P.same_results(res, single)
        assert all(r["stats"]["sharded_windows"] == r["stats"]["windows"] > 0 for r in res)


@pytest.mark.parametrize("seed", range(0, 192, 16))
def test_fuzz_slice_with_wide_groups(seed):
    with P.knobs(**WIDE):
        F.test_fuzz_case(seed, 3 if seed % 32 else 2)


# ---- k_dseed: windows of a chosen size on a settled table ---------------------------------------------------------------

def _fresh_points(seed, centres_seed, n, d, g):
    centres = np.random.default_rng(centres_seed).uniform(0.1, 0.9, (g, d))  # (make_blobs draws its centres first)
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.clip(centres[rng.integers(0, g, n)] + rng.normal(0.0, 0.01, (n, d)), 0.0, 1.0))


@pytest.fixture(scope="module")
def settled():
    """A table of 1 100 microclusters (the policy starts a call at the early window from 1 024 rows on) built by the default
    path, as a checkpoint; 20 000 fresh points of the same populations; the oracle's state after both."""
    from oracle import oracle as O
    n0, n, d, g = 30_000, 20_000, 20, 1100
    cfg = scenarios.params_to_config(scenarios.blob_params(n0))
    X, Y = scenarios.make_blobs(77, n0, d, g), _fresh_points(7707, 77, n, d, g)
    base = H._hdd(cfg)
    base.online_microcluster_maintenance(X, 0)
    state = base.get_state()
    o = O.OracleHDDStream(cfg)
    o.online_microcluster_maintenance(X, 0)
    H._check_against_oracle(base, o)
    o.online_microcluster_maintenance(Y, 0, reset_param=False)
    return cfg, X, Y, state, o


@pytest.mark.parametrize("lookahead", [2, 3])  # off, always
@pytest.mark.parametrize("B", [1009, 4097, 16400])
def test_dseed_window_sizes(settled, B, lookahead):
    """64, 257 and 1 025 records: one lane short of a wave's trip, one record into the fifth, one into the third group of eight."""
    cfg, X, Y, state, o = settled
    h = H._hdd(cfg, window=B, early_window=B, lookahead=lookahead, sequential=1)  # (sequential = 1: windows only)
    h.set_state(state)
    h._set_dataset_dependent_parameters(X)  # (mu of the first timepoint)
    s0 = h.stats()
    h.online_microcluster_maintenance(Y, 0, reset_param=False)
    s1 = h.stats()
    H._check_against_oracle(h, o)
    print("B %d lookahead %d: %d windows, %d truncated, %d rounds" % (
        B, lookahead, s1["windows"] - s0["windows"], s1["truncated"] - s0["truncated"], s1["rounds"] - s0["rounds"]))
    assert s1["seq_points"] == s0["seq_points"] and s1["rounds"] > s0["rounds"]  # windows, validated by k_dseed's rounds
    if s1["truncated"] == s0["truncated"]:
        assert s1["windows"] - s0["windows"] == -(-len(Y) // B)  # every window of the size that was asked for


def test_dseed_largest_window():
    """49 152 points: 3 072 records, 48 per lane.  The window policy takes that size from 4 096 microclusters on, which puts the
    oracle out of reach of a quick test (20 s per 100 000 points); the referee is the sequential kernel (k_seq_g: no windows,
    no k_dseed, no k_decide - itself pinned to the oracle by tests/test_sequential.py) on the same checkpoint."""
    n0, B, d, g = 450_000, 49152, 20, 4500
    n = B + 1000
    cfg = scenarios.params_to_config(scenarios.blob_params(n0))
    X, Y = scenarios.make_blobs(78, n0, d, g), _fresh_points(7808, 78, n, d, g)
    base = H._hdd(cfg)
    base.online_microcluster_maintenance(X, 0)
    state = base.get_state()
    assert len(state["pcore_id"]) + len(state["outlier_id"]) >= 4096

    def resume(**tuning):
        h = H._hdd(cfg, **tuning)
        h.set_state(state)
        h._set_dataset_dependent_parameters(X)
        s0 = h.stats()
        h.online_microcluster_maintenance(Y, 0, reset_param=False)
        return h, s0, h.stats()

    ref, r0, r1 = resume(sequential=2)
    assert r1["seq_points"] - r0["seq_points"] == n and r1["windows"] == r0["windows"]
    for lookahead in (2, 3):  # off, always
        h, s0, s1 = resume(window=B, early_window=B, lookahead=lookahead, sequential=1)
        PS._same_state(h, ref)
        print("lookahead %d: %d windows, %d truncated, %d rounds" % (
            lookahead, s1["windows"] - s0["windows"], s1["truncated"] - s0["truncated"], s1["rounds"] - s0["rounds"]))
        assert s1["seq_points"] == s0["seq_points"] and s1["rounds"] > s0["rounds"]
        # the settled table commits its windows in full: the first one held 49 152 points
        assert s1["truncated"] == s0["truncated"] and s1["windows"] - s0["windows"] == 2
