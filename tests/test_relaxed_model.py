"""The RELAXED multi-GPU mode (cc_comm_set_relaxed: online_relaxed, k_rel_delta / k_rel_merge / k_rel_promote / k_rel_collect,
k_sum_ranks) against its CPU model (tests/relaxed_model.py: DESIGN.md section 6 (3) restated on the oracle), bit for bit, on
in-process groups of handles on one GPU - the transport whose summation order the model can state - and, for a world of one,
on a one-rank RCCL group (ncclAllReduce of one rank adds nothing).

Per case every rank is compared with the model: uid and path per point (the first differing point is named), both lists in
order with id, uid, w, cf1, cf2, cen and pref, both id counters, and cc_relaxed_stats' super_steps, minibatch_points and
deferred_points.  No tolerances: the model does the same operations in the same order.

The cases are table_util.RELAXED_TABLES (injected tables and points laid out per rank; tests/test_relaxed_model_cpu.py shows
on the model alone that each holds what it exists for): promotions only the merge makes in a table where each thread of
k_rel_promote owns three rows; promotions a rank makes and the merge refuses, and the reverse; merged variances exactly on delta_sq; heavy outliers
that absorb nothing and stay; set-aside points on the pass
and wave boundaries of k_rel_collect, a rank that sets nothing aside and one that sets everything aside; centroids that a
merge moves past a neighbouring row under pruned scans; tainted tables; a stream with decay, downgrades and deletions between
the relaxed phases.  Widths 3 (below the ladder), 8, 13 and 37 (padded operands), 20, 40, 64; groups of 1, 2, 3, 4 and 8 ranks,
N no multiple of the world, N below it, a last rank with an empty shard; mini-batches of 64, 256, 2 500 and beyond the shard;
the library's own tuning and pruning forbidden (CHRONOCLUST_HIP_PRUNE=0)."""
import threading

import numpy as np
import pytest

import relaxed_model as R
import scenarios
import table_util as T
from test_pruned_scan import _env

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

MODES = {"default": {}, "prune0": dict(CHRONOCLUST_HIP_PRUNE=0), "prune2": dict(CHRONOCLUST_HIP_PRUNE=2)}

_cases, _models = {}, {}


def _case(name):
    if name not in _cases:
        _cases[name] = T.build_relaxed(name)
    return _cases[name]


def _model(name, world=None, n=None, minibatch=None):
    """(case with its first n points, the model's result) for a group of `world` ranks; the case's own layout (and its
    structure check) where nothing else is asked for.  Computed once per (case, group)."""
    key = (name, world, n, minibatch)
    if key not in _models:
        case = _case(name)
        if n is not None:
            case = case[:3] + (np.ascontiguousarray(case[3][:n]),) + case[4:]
        res = T.model_relaxed(case, world, minibatch)
        if world is None and n is None and minibatch is None:
            T.check_relaxed(case, res)
        _models[key] = (case, res)
    return _models[key]


class _Lists(object):
    """What same_lists reads of an oracle, from a model state."""

    def __init__(self, state):
        self.state, self.counters = state, tuple(state["counters"])

    def table(self, kind):
        return self.state["pcore" if kind == 0 else "outlier"]


def same_relaxed(h, labels, rstats, exp, rank, what):
    """One rank against the model: labels per point, both lists, the id counters, the statistics."""
    uid, path = labels
    for key, a, b in (("uid", uid, exp["uid"]), ("path", path, exp["path"])):
        diff = T._first_diff(a, b)
        assert diff is None, "%s %s per point (library / model): %s" % (what, key, diff)
    T.same_lists(h, _Lists(exp["state"]), what)
    want = dict(super_steps=exp["stats"]["super_steps"], minibatch_points=exp["stats"]["minibatch_points"][rank],
                deferred_points=exp["stats"]["deferred_points"])
    got = {k: rstats[k] for k in want}
    assert got == want, "%s relaxed_stats %r / %r" % (what, got, want)


def run_group(case, world, minibatch, mode="default"):
    """The case on an in-process group, a world of one on a one-rank RCCL group: (handles - the caller closes them -,
    [(labels, relaxed_stats, stats)] by rank)."""
    pcores, outliers, par, X, meta = case

    def work(h, rank):
        T.fill_handle(h, par, pcores, outliers)
        h.comm_set_relaxed(minibatch)
        labels = h.online(X)
        return labels, h.relaxed_stats(), h.stats()

    with _env(**MODES[mode]):
        if world > 1:
            return T._run_group(world, work)
        # a group of one exists over RCCL only (an in-process "group" of one handle is no group: cc_comm_set_relaxed refuses it)
        from chronoclust_amd import _lib
        h = _lib.Handle(0)
        try:
            h.comm_init_rccl(_lib.comm_unique_id(), 0, 1)
            return [h], [work(h, 0)]
        except BaseException:
            h.close()
            raise


def check_group(name, mode="default", world=None, n=None, minibatch=None):
    case, exp = _model(name, world, n, minibatch)
    world, minibatch = world or case[4]["world"], minibatch or case[4]["minibatch"]
    hs, results = run_group(case, world, minibatch, mode)
    try:
        for rank in range(world):
            labels, rstats, stats = results[rank]
            same_relaxed(hs[rank], labels, rstats, exp, rank, "%s [%s] rank %d of %d, mini-batch %d" % (name, mode, rank, world, minibatch))
            if case[4]["tainted"] or mode == "prune0":
                assert stats["scan_p_launches"] == 0, stats
        return [r[2] for r in results]
    finally:
        for h in hs:
            h.close()


SMALL_CLEAN = [n for n in T.RELAXED_TABLES if n.startswith(("divergence-", "promotions-small-", "threshold-"))]
SMALL_TAINTED = [n for n in T.RELAXED_TABLES if n.startswith(("tainted-2x150", "victims-"))]
LARGE_CLEAN = [n for n in T.RELAXED_TABLES if n.startswith(("promotions-3x2500", "compaction-"))]
LARGE_TAINTED = [n for n in T.RELAXED_TABLES if n.startswith("tainted-3x700")]
MOVING = [n for n in T.RELAXED_TABLES if n.startswith("moving-")]
assert len(SMALL_CLEAN) + len(SMALL_TAINTED) + len(LARGE_CLEAN) + len(LARGE_TAINTED) + len(MOVING) == len(T.RELAXED_TABLES)


@pytest.mark.parametrize("mode", ["default", "prune0"])
@pytest.mark.parametrize("name", SMALL_CLEAN + SMALL_TAINTED + LARGE_CLEAN + LARGE_TAINTED)
def test_relaxed_case_against_model(name, mode):
    check_group(name, mode)


@pytest.mark.parametrize("mode", ["default", "prune0", "prune2"])
@pytest.mark.parametrize("name", MOVING)
def test_moving_centroids_under_pruned_scans_against_model(name, mode):
    """2 048 pcores, nine merges, 64 probes whose nearest row is another one after the merge before them: whatever the scans
    derive from the table (padded operand copies, the half-precision prefix table, versions, carried candidates) must not
    outlive a merge.  Unless pruning is forbidden the pruned chain runs (the launch counter says so)."""
    stats = check_group(name, mode)
    print("%s [%s]: scan_p_launches %r, windows %r" % (name, mode, [s["scan_p_launches"] for s in stats], [s["windows"] for s in stats]))
    if mode != "prune0":                                         # (2 048 rows: the library's own policy prunes too)
        assert all(s["scan_p_launches"] > 0 for s in stats), stats


# the same points in other groups: (world, points, mini-batch) - one rank, N no multiple of the world, fewer points than
# ranks, a last rank with an empty shard (49 points on 8 ranks: shards of 7), a mini-batch beyond the shard
GROUPS = [(1, 300, 64), (2, 299, 64), (3, 300, 256), (8, 299, 64), (8, 5, 64), (8, 49, 2500), (2, 300, 1000)]


@pytest.mark.parametrize("world,n,minibatch", GROUPS)
@pytest.mark.parametrize("d", T.RELAXED_DIMS)
def test_tainted_table_in_other_groups_against_model(d, world, n, minibatch):
    check_group("tainted-2x150x%d" % d, "default", world, n, minibatch)


@pytest.mark.parametrize("world,n,minibatch", [(1, 600, 64), (2, 599, 256), (8, 600, 64), (8, 7, 64), (4, 9, 2500)])
@pytest.mark.parametrize("d", T.RELAXED_DIMS)
def test_clean_table_in_other_groups_against_model(d, world, n, minibatch):
    check_group("promotions-small-3x200x%d" % d, "default", world, n, minibatch)


def test_group_of_one_rank_over_rccl_against_model():
    """ncclAllReduce through the dlopen'ed library, communicator of one rank: the model with a world of one."""
    from chronoclust_amd import _lib
    name = "promotions-3x2500x8"
    case, exp = _model(name, 1, None, 2500)
    pcores, outliers, par, X, meta = case
    h = _lib.Handle(0)
    try:
        h.comm_init_rccl(_lib.comm_unique_id(), 0, 1)
        assert h.comm_info() == dict(rank=0, world=1, transport="rccl")
        T.fill_handle(h, par, pcores, outliers)
        h.comm_set_relaxed(2500)
        labels = h.online(X)
        same_relaxed(h, labels, h.relaxed_stats(), exp, 0, "%s over RCCL, one rank" % name)
    finally:
        h.close()


@pytest.mark.parametrize("world,minibatch", [(3, 256), (2, 2500)])
def test_decay_stream_against_model(world, minibatch):
    """Timepoints 0, 1, 3 through HDDStream with lambda = 0.5, drift and churn: fractional weights, downgrades and deletions
    between the relaxed phases.  After every timepoint every rank holds the model's labels, lists, counters and statistics,
    and its final clusters are the oracle's offline phase on the model's table, members in merge order."""
    Xs = scenarios.make_blob_timepoints(T.RELAXED_DECAY, raw=True)
    exp = R.relaxed_stream(T.relaxed_decay_config(), Xs, T.RELAXED_DECAY_DAYS, world, minibatch)
    from chronoclust_amd import _lib
    from chronoclust_amd.clustering.hddstream import HDDStream
    streams = [HDDStream(T.relaxed_decay_config()) for _ in range(world)]
    _lib.comm_init_local([s._h for s in streams])
    errors = [None] * world

    def work(rank):
        s = streams[rank]
        try:
            s._h.comm_set_relaxed(minibatch)
            for t, (X, day) in enumerate(zip(Xs, T.RELAXED_DECAY_DAYS)):
                s.online_microcluster_maintenance(X, day)
                what = "decay stream, timepoint %d (day %d), rank %d of %d" % (t, day, rank, world)
                same_relaxed(s._h, (s.labels_uid, s.labels_path), s._h.relaxed_stats(), exp[t], rank, what)
                members = [[int(x) for x in c.members_in_merge_order] for c in s.final_clusters]
                assert members == exp[t]["members"], "%s: members in merge order differ" % what
        except BaseException as e:  # noqa: BLE001 - reported after the join
            errors[rank] = e
            try:
                s._h.comm_destroy()
            except Exception:
                pass

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for e in errors:
        if e is not None:
            raise e


def test_relaxed_mode_refuses_65_dimensions_on_every_rank_and_works_at_64_afterwards():
    """online_range refuses no_create beyond CC_WINDOW_MAX_DIM before any collective runs: every rank gets the library's error,
    every thread joins, and the same handles - in a fresh group, the refusal gives the old one up - cluster 64 dimensions."""
    from chronoclust_amd import _lib
    world = 3
    case, exp = _model("tainted-2x150x64", world, None, 64)
    pcores, outliers, par, X, meta = case
    wide = np.ascontiguousarray(np.random.default_rng(5).uniform(0.1, 0.9, (30, 65)))
    hs = [_lib.Handle(0) for _ in range(world)]
    try:
        _lib.comm_init_local(hs)
        errors, results = [None] * world, [None] * world
        ready = threading.Barrier(world)

        def refuse(rank):
            h = hs[rank]
            arrived = False
            try:
                h.set_params(*par._replace(pi=65))
                h.comm_set_relaxed(64)
                h.points_upload(wide)
                ready.wait(60)                              # (every rank is refused by its own call, not by a peer's failure)
                arrived = True
                h.online_run()
            except BaseException as e:  # noqa: BLE001
                errors[rank] = e
                if not arrived:                             # (a rank refused after the barrier must not break it for a peer that
                    ready.abort()                           # is still on its way out of wait(): that peer would see the abort)

        threads = [threading.Thread(target=refuse, args=(r,)) for r in range(world)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(60)
        assert not any(th.is_alive() for th in threads), "a rank still waits for its peers"
        for rank, e in enumerate(errors):
            assert isinstance(e, ValueError) and "more than 64 dimensions" in str(e), "rank %d: %r" % (rank, e)

        for h in hs:
            try:
                h.comm_destroy()
            except Exception:
                pass
            h.reset()
        _lib.comm_init_local(hs)

        def work(rank):
            h = hs[rank]
            try:
                T.fill_handle(h, par, pcores, outliers)
                h.comm_set_relaxed(64)
                results[rank] = (h.online(X), h.relaxed_stats())
            except BaseException as e:  # noqa: BLE001
                errors[rank] = e
                try:
                    h.comm_destroy()
                except Exception:
                    pass

        errors = [None] * world
        threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        for e in errors:
            if e is not None:
                raise e
        for rank in range(world):
            same_relaxed(hs[rank], results[rank][0], results[rank][1], exp, rank, "64 dimensions after the refusal, rank %d" % rank)
    finally:
        for h in hs:
            h.close()
