"""Beyond 128 dimensions (128 < d <= CC_MAX_DIM = 1 024; hddstream.py:101-114 takes any d): the online phase runs on the
wide form of k_seq_g (a point's dimensions in blocks of 64) from the first point on, the offline phase on the
dimension-blocked k_eps_neighbours_blk, the tracker on k_assoc_tiled_blk, the device scaler on column blocks of 256 -
against the oracle like every other path (labels, both tables bit for bit, clusters in merge order), against a golden
recorded from the reference at d = 160, through app.run with a checkpoint, and the refusals that remain."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import scenarios
from golden_util import GOLDEN, StateDump
from test_hip_parity import _check_against_oracle, _hdd, _replay_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the golden's scenario: the same dict as tests/golden/make_golden_wide.py (the inputs are checked against the hashes it
# recorded)
D160 = dict(seed=160, n=1500, d=160, g=10, sigma=0.01, wide_dims=(12, 20), wide_sigma=0.08, timepoints=3, drift=0.01,
            churn=0.2, params=scenarios.blob_params(1500, param_epsilon=0.4, param_pi=150, param_upsilon=10.0,
                                                    param_omicron=0.0002, param_lambda=1.5))

FUZZ_DIMS = (129, 160, 200, 256, 300, 511, 512, 513, 700, 1024)


def _reset_logging():
    import logging
    root = logging.getLogger()
    for h in list(root.handlers):
        root.removeHandler(h)
        h.close()


def _labels(csv_path):
    df = pd.read_csv(csv_path, keep_default_na=False, dtype=str)
    return df["id"].to_numpy().astype(np.int64), df["cluster_id"].to_numpy().astype(str)


def _write_timepoints(Xs, where):
    files = []
    for t, X in enumerate(Xs):
        fn = os.path.join(where, "tp%d.csv" % t)
        pd.DataFrame(X, columns=["m%d" % i for i in range(X.shape[1])]).to_csv(fn, index=False)
        files.append(fn)
    return files


def test_the_accepted_width_is_1024():
    """CPU only: the C-ABI header, the Python binding and the policy's entry point agree on 1 024."""
    from chronoclust_amd import _lib
    with open(os.path.join(ROOT, "include", "chronoclust_hip.h")) as f:
        header = f.read()
    assert int(re.search(r"^#define CC_MAX_DIM (\d+)", header, re.M).group(1)) == _lib.MAX_DIM == 1024
    g = _lib.load().cc_policy_seq_rate_guess
    assert g(200, 300, 1, 1) > 0 and g(1024, 300, 1, 1) > 0
    assert g(1025, 300, 1, 1) < 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(len(FUZZ_DIMS)))
def test_any_dims_streams_fuzz(seed):
    """Ten seeded streams, one per width (512 / 513: the last width with two points per staged chunk and the first with
    one): anisotropic blobs (a few wide dimensions each, so that the pdim filter lets microclusters in) with an epsilon
    below to above a blob's radius (several microclusters per blob, tables of tens to thousands of rows), 2 % uniform
    noise, decay and deletion, two populations that end."""
    from oracle import oracle as O
    d = FUZZ_DIMS[seed]
    rng = np.random.default_rng(10240 + seed)
    g = int(rng.integers(4, 30))
    n = int(rng.choice([1500, 2000, 3000])) if d <= 512 else 1500
    sigma = float(rng.choice([0.004, 0.015, 0.03]))
    k = float((1.0, 2.0, 3.0, 4.0)[seed % 4])
    pi = 0 if seed % 2 == 0 else d - 3
    wide = np.zeros((g, d), dtype=bool)
    for i in range(g):
        wide[i, rng.choice(d, int(rng.integers(4, 9)), replace=False)] = True
    sig = np.where(wide, 0.08, sigma)
    eps = float(np.sqrt(float(rng.choice([0.5, 0.8, 1.5])) * (d * sigma * sigma / k + 6 * 0.0064)))
    cfg = scenarios.params_to_config(scenarios.blob_params(
        n, param_epsilon=eps, param_k=k, param_pi=pi, param_lambda=float(rng.choice([0.5, 2.0])), param_omicron=0.0003,
        promote_after=int(rng.choice([3, 10]))))
    h, o = _hdd(cfg), O.OracleHDDStream(cfg)
    centres = rng.uniform(0.1, 0.9, (g, d))
    for t in range(3):
        lab = rng.integers(0, g, n)
        X = np.clip(centres[lab] + rng.normal(0.0, 1.0, (n, d)) * sig[lab], 0.0, 1.0)
        noise = rng.random(n) < 0.02
        X[noise] = rng.random((int(noise.sum()), d))
        X = np.ascontiguousarray(X)
        h.online_microcluster_maintenance(X, t)
        o.online_microcluster_maintenance(X, t)
        _check_against_oracle(h, o)
        s = h.stats()
        assert s["seq_g_points"] == n and s["windows"] == 0  # (every point on k_seq_g, no window)
        centres = np.clip(centres + rng.normal(0.0, 0.004, centres.shape), 0.0, 1.0)
        if t == 0:
            centres, sig, g = centres[: max(1, g - 2)], sig[: max(1, g - 2)], max(1, g - 2)  # (populations end)


def _grouped_centres(rng, d, n_groups=24):
    """Blob centres in groups of 1-7 around group centres: within a group ~1-3 apart (0.06 per dimension, plus 0-24
    dimensions in which the group's blobs differ by ~0.25, so that PreDeCon's pdim varies from group to group), between
    groups ~3 (d = 200) to ~6 (d = 700) apart."""
    sizes = rng.integers(1, 8, n_groups)
    supers = rng.uniform(0.25, 0.75, (n_groups, d))
    centres = []
    for gi, sz in enumerate(sizes):
        spread = rng.choice(d, int(rng.integers(0, 25)), replace=False)
        for _ in range(sz):
            c = supers[gi] + rng.normal(0.0, 0.06, d)
            c[spread] += rng.normal(0.0, 0.25, len(spread))
            centres.append(c)
    return np.clip(np.array(centres), 0.05, 0.95)


@pytest.mark.gpu
@pytest.mark.parametrize("d,ups_eps", [(200, 2.5), (700, 4.0)])
def test_any_dims_offline_intermediates_against_oracle(d, ups_eps):
    """Core flags, |N_eps|, PreDeCon pdim and |N_w| per pcore (predecon.py:136-217) with neighbourhoods that are neither
    empty nor complete: one pcore per blob, ~90-110 of them (two 64-lane words of q's, full CC_EPS_TP tiles of p rows and
    a partial one), upsilon * epsilon between the distances within a group of blobs and those between groups - the
    dimension-blocked k_eps_neighbours_blk.  Anisotropic blobs (pi < d), k = 3."""
    from oracle import oracle as O
    n = 4000
    rng = np.random.default_rng(d)
    eps = float(np.sqrt(2.0 * (0.9 * d * 1e-4 / 3 + 0.1 * d * 0.06 ** 2)))  # (twice a blob's squared projected radius)
    cfg = scenarios.params_to_config(scenarios.blob_params(n, param_epsilon=eps, param_pi=d - 10, param_k=3,
                                                            param_upsilon=ups_eps / eps, param_omicron=0.0002,
                                                            param_lambda=1.5))
    h, o = _hdd(cfg), O.OracleHDDStream(cfg)
    centres = _grouped_centres(rng, d)
    g = len(centres)
    wide = rng.random((g, d)) < 0.1
    for t in range(2):
        lab = rng.integers(0, g, n)
        X = np.ascontiguousarray(np.clip(centres[lab] + rng.normal(0.0, 1.0, (n, d)) * np.where(wide[lab], 0.06, 0.01),
                                         0.0, 1.0))
        h.online_microcluster_maintenance(X, t)
        o.online_microcluster_maintenance(X, t)
        _check_against_oracle(h, o)
        _, info = h._h.offline(dumps=True)
        for key in ("core", "pdim", "nn", "nw"):
            np.testing.assert_array_equal(info[key], o.offline_dump[key], err_msg="%s t=%d" % (key, t))
        nn = o.offline_dump["nn"]
        mp = len(nn)
        assert mp > 64 and mp % 32 != 0  # (more than one word of q's; a partial tile of p rows)
        assert len(np.unique(nn)) > 2 and np.any((nn > 1) & (nn < mp)) and np.any(nn == 1)
        assert len(np.unique(o.offline_dump["pdim"])) > 2 and len(h.final_clusters) > 1


@pytest.mark.gpu
def test_any_dims_assoc_argmin_against_oracle():
    """TrackByHistoricalAssociation's nearest previous cluster (cluster_tracker.py:120-144) beyond 128 dimensions:
    k_assoc_tiled_blk with the unit operand (k = 4) and the division (k = 3), more than one workgroup row of current
    pcores (mc > 256), several sub-ranges of previous ones, and exact ties that decide the argmin: previous pcores 0, 1
    and mp / 2 are copies of one another (the same staged tile; another tile and another sub-range once mp >= 64), and
    some current pcores lie on that copy or right beside it - the first copy must win (strict < within the tiles, the
    sub-ranges folded in ascending order)."""
    from chronoclust_amd import _lib
    from oracle import oracle as O
    rng = np.random.default_rng(3)
    hd = _lib.Handle(0)
    for mc, mp, d, k in ((1, 1, 129, 4.0), (37, 129, 256, 3.0), (300, 500, 777, 4.0), (300, 400, 777, 3.0),
                         (64, 2000, 1024, 3.0), (260, 300, 1024, 4.0)):
        hd.set_params(0.01, 0.01, k, 0.5, 1.0, 0.0, 0.1, 0.01, 0.1, d)
        cur = rng.random((mc, d))
        pref = np.where(rng.random((mc, d)) < 0.5, k, 1.0)
        prev = rng.random((mp, d))
        prev[mp // 2] = prev[0]
        if mp > 2:
            prev[1] = prev[0]
        tied = rng.choice(mc, min(mc, 4), replace=False)
        cur[tied[0]] = prev[0]                                                    # distance 0 to every copy
        cur[tied[1:]] = prev[0] + rng.normal(0.0, 1e-3, (len(tied) - 1, d))       # the same non-zero distance to each
        gi, gd = hd.assoc_argmin(cur, pref, prev)
        oi, od = O.assoc_argmin(cur, pref, prev)
        np.testing.assert_array_equal(gi, oi)
        assert np.array_equal(gd, od)
        assert (gi[tied] == 0).all() and gd[tied[0]] == 0.0 and (gd[tied[1:]] > 0.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n,d", [(1000, 257), (5003, 300), (100, 1024)])
def test_any_dims_device_scaler_matches_the_restated_minmaxscaler(n, d):
    """cc_col_minmax (column blocks of 256) / cc_points_upload_scaled / cc_points_download against
    chronoclust_amd.scaling.scaler.Scaler's numpy arithmetic, with a zero-range column and a NaN that the fit ignores in
    the last column block."""
    from chronoclust_amd import _lib
    from chronoclust_amd.scaling.scaler import Scaler
    rng = np.random.default_rng(n + d)
    X = rng.normal(3.0, 50.0, (n, d)) * rng.uniform(1e-3, 1e3, d)
    X[:, 1] = 7.25          # zero range: scale_ stays 1
    X[:, d - 2] = -1.5      # (one in the last block too)
    X[3, 0] = X[:, 0].max() + 1.0
    hd = _lib.Handle(0)
    mn, mx = hd.col_minmax(X)
    np.testing.assert_array_equal(mn, X.min(axis=0))
    np.testing.assert_array_equal(mx, X.max(axis=0))
    Xn = X.copy()
    Xn[2, d - 1] = np.nan    # ignored by the fit, like np.nanmin / np.nanmax
    mn2, mx2 = hd.col_minmax(Xn)
    np.testing.assert_array_equal(mn2, np.nanmin(Xn, axis=0))
    np.testing.assert_array_equal(mx2, np.nanmax(Xn, axis=0))
    ref = Scaler()
    ref.fit_scaler(X)
    hd.points_upload_scaled(X, ref.scale_, ref.min_)
    scaled = hd.points_download(d)
    assert np.array_equal(scaled, ref.scale_data(X))
    back = hd.points_download(d, ref.scale_, ref.min_)
    assert np.array_equal(back, ref.reverse_scaling(ref.scale_data(X)))


def _d160_inputs(dump):
    import hashlib
    Xs = scenarios.make_blob_timepoints(D160)
    for t, X in enumerate(Xs):
        sha = np.frombuffer(hashlib.sha256(np.ascontiguousarray(X).tobytes()).digest(), dtype=np.uint8)
        assert (sha == dump.get(t, "xsha")).all(), "numpy Generator stream changed: regenerate the golden"
    return Xs


@pytest.mark.gpu
def test_d160_golden_replay():
    """The reference's state after every timepoint at d = 160 (tests/golden/make_golden_wide.py): labels, both tables bit
    for bit, clusters in merge order, replayed through HDDStream."""
    dump = StateDump(os.path.join(GOLDEN, "blob_d160.npz"))
    assert max(int(dump.get(t, "n_clusters")[0]) for t in range(dump.n_timepoints)) >= 2
    assert max(len(dump.get(t, "pcore_id")) for t in range(dump.n_timepoints)) >= 1
    h = _replay_dump(dump, _d160_inputs(dump), scenarios.params_to_config(D160["params"]))
    s = h.stats()
    assert s["seq_g_points"] == D160["n"] and s["windows"] == 0


@pytest.mark.gpu
def test_d160_end_to_end(tmp_path):
    """The d = 160 scenario through app.run: result.csv bytes and per-point cluster ids of the recorded reference run."""
    from chronoclust_amd import app
    z = np.load(os.path.join(GOLDEN, "blob_d160.npz"))
    Xs = scenarios.make_blob_timepoints(D160, raw=True)
    files = _write_timepoints(Xs, str(tmp_path))
    out = os.path.join(str(tmp_path), "out")
    os.makedirs(out)
    try:
        app.run(data=files, output_directory=out, normalise_data=False, **D160["params"])
    finally:
        _reset_logging()
    assert open(os.path.join(out, "result.csv"), "rb").read() == z["result_csv"].tobytes()
    for t in range(len(Xs)):
        ids, cl = _labels(os.path.join(out, "cluster_points_D%d.csv" % t))
        assert (ids == np.arange(len(ids))).all()
        assert (cl == z["t%d_cluster_id" % t]).all()


@pytest.mark.gpu
def test_restore_program_continues_exactly_at_d200(tmp_path):
    """Stop after two of four timepoints at d = 200, restart with restore_program=True: every output file equals that of
    an uninterrupted run."""
    from chronoclust_amd import app
    import chronoclust_amd.app as A
    sc = dict(seed=200, n=1000, d=200, g=8, sigma=0.01, timepoints=4, drift=0.01, churn=0.25,
              params=scenarios.blob_params(1000, param_epsilon=0.12, param_omicron=0.0002, param_lambda=1.5))
    files = _write_timepoints(scenarios.make_blob_timepoints(sc, raw=True), str(tmp_path))
    whole, resumed = os.path.join(str(tmp_path), "whole"), os.path.join(str(tmp_path), "resumed")
    os.makedirs(whole)
    os.makedirs(resumed)

    class Stop(Exception):
        pass

    orig = A.save_program_state

    def save_and_maybe_stop(h, o, ta, tl):
        orig(h, o, ta, tl)
        if h.last_data_timestamp == 1:
            raise Stop()

    try:
        app.run(data=files, output_directory=whole, **sc["params"])
        _reset_logging()
        A.save_program_state = save_and_maybe_stop
        try:
            app.run(data=files, output_directory=resumed, **sc["params"])
        except Stop:
            pass
        finally:
            A.save_program_state = orig
        _reset_logging()
        assert open(os.path.join(resumed, "result.csv")).read() != open(os.path.join(whole, "result.csv")).read()
        app.run(data=files, output_directory=resumed, restore_program=True, **sc["params"])
    finally:
        _reset_logging()
    names = ["result.csv"] + ["cluster_points_D%d.csv" % t for t in range(sc["timepoints"])]
    for name in names:
        with open(os.path.join(whole, name), "rb") as a, open(os.path.join(resumed, name), "rb") as b:
            assert a.read() == b.read(), name
    ids, cl = _labels(os.path.join(whole, "cluster_points_D%d.csv" % (sc["timepoints"] - 1)))
    assert len(set(cl) - {"None"}) >= 1  # (the comparison is about clustered points)


@pytest.mark.gpu
def test_wider_than_1024_is_refused():
    """d = 1 025: the handle, the scaler's reduction and the scaled upload all refuse it, naming the limit."""
    from chronoclust_amd import _lib
    from chronoclust_amd.clustering.hddstream import HDDStream
    X = np.random.default_rng(0).random((40, 1025))
    with pytest.raises(ValueError, match="1024"):
        HDDStream(scenarios.params_to_config(scenarios.blob_params(40))).online_microcluster_maintenance(X, 0)
    hd = _lib.Handle(0)
    with pytest.raises(ValueError, match="1024"):
        hd.col_minmax(X)
    with pytest.raises(ValueError, match="1024"):
        hd.points_upload_scaled(X, np.ones(1025), np.zeros(1025))


@pytest.mark.gpu
def test_wide_points_are_refused_in_a_group_beyond_128():
    """d = 200 in an in-process group of two: the call fails before any collective, as it does from 65 dimensions on."""
    from chronoclust_amd import _lib
    from chronoclust_amd.clustering.hddstream import HDDStream
    n, d = 500, 200
    cfg = scenarios.params_to_config(scenarios.blob_params(n))
    s, peer = HDDStream(cfg), HDDStream(cfg)
    _lib.comm_init_local([s._h, peer._h])
    with pytest.raises(ValueError, match="dimensions"):  # (CC_ERR_BAD_ARG maps to ValueError)
        s.online_microcluster_maintenance(scenarios.make_blobs(3, n, d, 5), 0)
