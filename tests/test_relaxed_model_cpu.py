"""The CPU model of the relaxed multi-GPU mode (tests/relaxed_model.py) on its own, no GPU: the oracle's two additions behave
as documented and leave the reference's loop as it was, and every case of table_util.RELAXED_TABLES holds what it was built
for - the structure conditions of table_util.check_relaxed on the MODEL's result, as check_online does for the online cases.
Each case prints the counts behind its conditions and the model's time (oracle time included); tests/test_relaxed_model.py
compares the library with the same results bit for bit."""
import time

import numpy as np
import pytest

import relaxed_model as R
import scenarios
import table_util as T

ORACLE_SECONDS = 2.0  # per case, on the CPU


def test_no_create_sets_aside_and_leaves_the_lists_untouched():
    case = T.build_online("stale-31+33x5")
    pcores, outliers, par, X, meta = case
    plain = T.oracle_online(case)
    assert (plain["path"] == 2).any() and (plain["uid"] >= 0).all() and not (plain["path"] & 8).any()   # the default: as ever
    o = T.make_oracle(par, pcores, outliers)
    assert not o.no_create
    before = R.state_of(o)
    o.no_create = True
    o.online_microcluster_maintenance(X, 0, reset_param=False, offline=False)
    aside = o.labels_uid == -1
    assert aside.any() and (o.paths[aside] == 8).all() and not (o.paths[~aside] & 8).any() and (o.paths != 2).all()
    after = R.state_of(o)
    assert after["counters"][1] == before["counters"][1]
    assert len(after["pcore"]["w"]) + len(after["outlier"]["w"]) == len(pcores) + len(outliers)
    # without the points that were set aside the plain loop does exactly the same
    o2 = T.make_oracle(par, pcores, outliers)
    o2.online_microcluster_maintenance(X[~aside], 0, reset_param=False, offline=False)
    assert np.array_equal(o2.labels_uid, o.labels_uid[~aside]) and np.array_equal(o2.paths, o.paths[~aside])
    for kind in (0, 1):
        a, b = o.table(kind), o2.table(kind)
        for key in a:
            assert np.array_equal(a[key], b[key]), (kind, key)


def test_set_counters_overrides_what_injection_derived():
    pcores, outliers, par, X, meta = T.build_online("stale-31+33x5")
    o = T.make_oracle(par, pcores, outliers)
    p0, o0 = o.counters
    assert p0 == int(pcores.id.max()) + 1 and o0 == int(outliers.uid.max()) + 1
    o.set_counters(p0 + 1000, o0 + 5000)
    assert o.counters == (p0 + 1000, o0 + 5000)
    far = np.full((1, X.shape[1]), 50.0)
    o.online_microcluster_maintenance(far, 0, reset_param=False, offline=False)
    assert o.labels_uid[0] == o0 + 5000 and o.counters == (p0 + 1000, o0 + 5001)


def test_super_step_schedule():
    assert R.super_steps(2500, 2500) == [(0, 2048), (2048, 2500)]
    assert R.super_steps(5000, 2500) == [(0, 2048), (2048, 4548), (4548, 5000)]
    assert R.super_steps(300, 64) == [(a, min(300, a + 64)) for a in range(0, 300, 64)]
    assert R.super_steps(10000, 65536) == [(0, 2048), (2048, 6144), (6144, 10000)]
    assert R.super_steps(0, 64) == []


@pytest.mark.parametrize("name", list(T.RELAXED_TABLES))
def test_relaxed_case_holds_what_it_was_built_for(name):
    case = T.build_relaxed(name)
    pcores, outliers, par, X, meta = case
    rows = (len(pcores) if pcores is not None else 0) + (len(outliers) if outliers is not None else 0)
    assert rows <= 2148 and len(X) <= 7500
    t0 = time.time()
    res = T.model_relaxed(case)
    seconds = time.time() - t0
    counts = T.check_relaxed(case, res)
    print("%s: %d rows, %d points, world %d, mini-batch %d, %s; %s; model (oracle included) %.2f s" % (
        name, rows, len(X), meta["world"], meta["minibatch"], res["stats"], counts, seconds))
    assert (res["uid"] >= 0).all() and not (res["path"] & 8).any()
    assert seconds < ORACLE_SECONDS


@pytest.mark.parametrize("world,n,minibatch", [(1, 300, 64), (2, 299, 64), (8, 5, 64), (8, 49, 2500), (4, 9, 64), (3, 1, 64)])
def test_model_on_uneven_and_empty_shards(world, n, minibatch):
    """N no multiple of the world, fewer points than ranks, a last rank without points: every point labelled once, the
    schedule that of the longest shard, every rank's mini-batch points its shard."""
    case = T.build_relaxed("tainted-2x150x8")
    case = case[:3] + (np.ascontiguousarray(case[3][:n]),) + case[4:]
    res = T.model_relaxed(case, world, minibatch)
    shard = -(-n // world)
    assert (res["uid"] >= 0).all() and res["stats"]["super_steps"] == len(R.super_steps(shard, minibatch))
    assert sum(res["stats"]["minibatch_points"]) == n
    assert res["stats"]["minibatch_points"] == [max(0, min(n, (r + 1) * shard) - min(n, r * shard)) for r in range(world)]


def test_decay_stream_has_fractional_weights_downgrades_deletions_and_merged_promotions():
    Xs = scenarios.make_blob_timepoints(T.RELAXED_DECAY, raw=True)
    t0 = time.time()
    out = R.relaxed_stream(T.relaxed_decay_config(), Xs, T.RELAXED_DECAY_DAYS, 3, 256)
    seconds = time.time() - t0
    down = sum(r["boundary"]["downgraded"] for r in out)
    gone = sum(r["boundary"]["deleted"] for r in out)
    promoted = [sum(len(s["info"]["promoted"]) for s in r["steps"] if s["info"] is not None) for r in out]
    w = np.concatenate([out[-1]["state"][k]["w"] for k in ("pcore", "outlier")])
    print("decay stream: downgraded %d, deleted %d, promoted by merges %r, clusters %r, set aside %r, fractional weights %d of %d; "
          "%.2f s" % (down, gone, promoted, [len(r["members"]) for r in out], [r["stats"]["deferred_points"] for r in out],
                      int((w != np.round(w)).sum()), len(w), seconds))
    assert down > 0 and gone > 0 and all(p > 0 for p in promoted) and (w != np.round(w)).any()
    assert all(len(r["members"]) > 1 for r in out) and seconds < ORACLE_SECONDS
    # no decay before the first timepoint: a microcluster's weight is the number of points labelled with it
    first = out[0]
    uid = np.concatenate([first["state"][k]["uid"] for k in ("pcore", "outlier")])
    w0 = np.concatenate([first["state"][k]["w"] for k in ("pcore", "outlier")])
    u, counts = np.unique(first["uid"], return_counts=True)
    order = np.argsort(uid)
    assert np.array_equal(uid[order], u) and np.array_equal(w0[order], counts.astype(np.float64))
