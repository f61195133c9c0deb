"""cc_assign (k_assign_scan + k_assign_decide) against the CPU oracle on the injected tables of tests/table_util.py: per
point a FRESH oracle that holds the table answers for that one point (tests/assign_util.py).  uid and path must be equal
per point bit for bit, the distance - where asked for - must be oracle.projected_distance of the reported row.  On these
cases the frozen answer differs from the sequential one at about a third of the points (tests/test_assign_cpu.py asserts it
on the oracle alone), so a call that runs the online phase cannot pass; and the table must be the same afterwards."""
import numpy as np
import pytest

import assign_util as A
import table_util as T
from pipeline_util import knobs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


def _handle(name, **env):
    """A handle that holds the case's table (created under the given knobs)."""
    from chronoclust_amd import _lib
    pcores, outliers, par = A.case(name)[:3]
    with knobs(**env):
        h = _lib.Handle(0)
    return T.fill_handle(h, par, pcores, outliers)


def _check(name, h=None, what=None, **env):
    own = h is None
    h = h if h is not None else _handle(name, **env)
    try:
        X = A.case(name)[3]
        got = h.assign(X, want_path=True, want_dist=True)
        A.same_assign(got, A.frozen(name), what or name)
        s = h.stats()
        assert s["assign_points"] == len(X), s
        return got, s
    finally:
        if own:
            h.close()


EDGES = ["stale-1+0x3", "stale-31+33x5", "stale-32+0x8", "stale-0+129x13", "stale-127+128x14"]
TIES = ["lattice-33+33x3", "lattice-128+127x8", "lattice-129+64x13"]
WIDTHS = ["stale-300x80", "lattice-200+100x80", "stale-filter-150x200", "lattice-100+64x200", "stale-filter-33+31x129",
          "stale-20+10x1024"]
TAINTED = ["victims-k4-64x13", "victims-k4-50x200", "victims-k3-200x14", "stale-k0.5-600x32", "victims-outliers-k3-500x40"]


@pytest.mark.parametrize("name", EDGES + TIES + WIDTHS + TAINTED)
def test_assign_against_the_frozen_oracle(name):
    rows, points = A.rows_points(name)
    assert rows * points <= 300000
    (uid, path, dist), s = _check(name)
    assert s["assign_launches"] == 1, s
    pcores, outliers, par, X, meta, idx = A.case(name)
    if meta["kind"] == "victims":  # the near row, not the victim's neighbour
        t = meta["rows"]
        assert np.array_equal(uid, t.uid[meta["R"][meta["pair"][idx]]]), name
        assert (path == (5 if meta["on_outliers"] else 0)).all(), np.unique(path)
    if name in ("stale-31+33x5", "stale-127+128x14", "stale-20+10x1024") + tuple(TIES):
        assert {0, 1, 2, 5} <= set(int(p) for p in np.unique(path)), np.unique(path)


def test_empty_table_single_point_and_no_points():
    from chronoclust_amd import _lib
    par, X = A.case("stale-31+33x5")[2:4]
    h = _lib.Handle(0)
    try:
        h.set_params(*par)
        uid, path, dist = h.assign(X, want_dist=True)      # an empty table: "new" everywhere
        assert (uid == -1).all() and (path == 2).all() and (dist == -1.0).all()
        assert h.count(_lib.PCORE) == 0 and h.count(_lib.OUTLIER) == 0 and h.counters() == (0, 0)
        uid, path, dist = h.assign(np.empty((0, 5)))        # n = 0 succeeds
        assert len(uid) == 0 and len(path) == 0 and dist is None
        s = h.stats()
        assert s["assign_points"] == 0 and s["assign_launches"] == 0, s
    finally:
        h.close()
    name = "stale-127+128x14"
    h = _handle(name)
    try:
        X, exp = A.case(name)[3], A.frozen(name)
        for i in (0, 77, len(X) - 1):                       # n = 1
            got = h.assign(X[i:i + 1], want_dist=True)
            A.same_assign(got, tuple(e[i:i + 1] for e in exp), "%s point %d alone" % (name, i))
        uid, path, dist = h.assign(X, want_path=False)      # the optional outputs left out
        assert path is None and dist is None
        A.same_assign((uid, None, None), exp, name + " uid only")
    finally:
        h.close()


@pytest.mark.parametrize("segments", [1, 2, 3])
def test_chunks_and_row_segments(segments):
    """500 points in 8 chunks of 64 (the last one partial), the rows in 1, 2 and 3 segments: the answers of the defaults."""
    name = "stale-127+128x14"
    got, s = _check(name, what="%s, chunks of 64, %d segments" % (name, segments),
                    CHRONOCLUST_HIP_ASSIGN_CHUNK=64, CHRONOCLUST_HIP_ASSIGN_SEGMENTS=segments)
    assert s["assign_points"] == 500 and s["assign_launches"] == 8, s
    default, s0 = _check(name)
    assert s0["assign_launches"] == 1, s0
    A.same_assign(got, default, "knobs against defaults")


def test_chunk_boundaries_off_the_point_tile():
    """Chunks of 100 points (no multiple of the 64-point tile) and of 1 point."""
    name = "lattice-129+64x13"
    got, s = _check(name, CHRONOCLUST_HIP_ASSIGN_CHUNK=100, CHRONOCLUST_HIP_ASSIGN_SEGMENTS=5)
    assert s["assign_launches"] == 3, s
    h = _handle(name, CHRONOCLUST_HIP_ASSIGN_CHUNK=1)
    try:
        X = A.case(name)[3][:9]
        A.same_assign(h.assign(X, want_dist=True), tuple(e[:9] for e in A.frozen(name)), name + " one point per chunk")
        assert h.stats()["assign_launches"] == 9
    finally:
        h.close()


def test_fifteen_hundred_rows_at_the_defaults():
    name = "lattice-1000+500x14"
    rows, points = A.rows_points(name)
    assert rows == 1500 and rows * points <= 300000
    _check(name)


def test_nothing_moved():
    """Both lists, the counters, the resident points' labels and every other field of cc_stats are the same after an assign;
    the online phase that follows is the sequential oracle's; a tainted handle stays tainted (pruning forced: no pruned
    scan is launched afterwards)."""
    from chronoclust_amd import _lib
    name = "stale-127+128x14"
    pcores, outliers, par, X, meta, _ = A.case(name)
    assert meta["tainted"]
    h = _handle(name, CHRONOCLUST_HIP_PRUNE=2)
    try:
        h.set_tuning(sequential=1)
        warm = np.ascontiguousarray(X[:5] + 100.0)          # far from every row: five new outliers, labels to keep
        h.online(warm)

        def snapshot():
            lists = [h.export(kind) for kind in (_lib.PCORE, _lib.OUTLIER)]
            return ([{k: v.tobytes() for k, v in t.items()} for t in lists], h.counters(),
                    tuple(a.tobytes() for a in h.labels_download()), h.stats())

        before = snapshot()
        tables = [T.Table.__new__(T.Table) for _ in range(2)]
        for t, kind in zip(tables, (_lib.PCORE, _lib.OUTLIER)):
            t.__dict__.update(h.export(kind))
        got = h.assign(X, want_dist=True)
        after = snapshot()
        assert before[0] == after[0], "a list changed"
        assert before[1] == after[1] and before[2] == after[2], "counters or resident labels changed"
        for key, val in before[3].items():
            if key not in ("assign_points", "assign_launches"):
                assert after[3][key] == val or (val != val and after[3][key] != after[3][key]), key
        assert after[3]["assign_points"] == len(X) and after[3]["assign_launches"] == 1
        # the answers against the table as it stands now (the injected rows and the five new outliers)
        sub = slice(None, None, 5)
        exp = A.frozen_answers(tables[0], tables[1], par, X[sub])
        A.same_assign(tuple(g[sub] for g in got), exp, name + " after an online call")
        # ... and the online phase goes on as if nothing had been asked
        o = T.make_oracle(par, pcores, outliers)
        o.online_microcluster_maintenance(warm, 0, reset_param=False, offline=False)
        o.online_microcluster_maintenance(X, 0, reset_param=False, offline=False)
        labels = h.online(X)
        T.same_online(h, (labels, None), dict(o=o, uid=o.labels_uid, path=o.paths), name + " online after assign")
        s = h.stats()
        assert s["windows"] > 0 and s["scan_p_launches"] == 0 and s["scan_u_launches"] == 0, s   # still tainted
    finally:
        h.close()


def test_errors():
    from chronoclust_amd import _lib
    name = "stale-31+33x5"
    X = A.case(name)[3]
    h = _handle(name)
    try:
        bad = X.copy()
        bad[17, 2] = np.nan
        with pytest.raises(ValueError, match="non-finite"):
            h.assign(bad)
        bad[17, 2] = np.inf
        with pytest.raises(ValueError, match="non-finite"):
            h.assign(bad)
        with pytest.raises(ValueError, match="bad argument"):
            h.assign(np.zeros((3, 6)))
        with pytest.raises(ValueError, match="bad argument"):
            h.assign(np.zeros((3, _lib.MAX_DIM + 1)))
        A.same_assign(h.assign(X, want_dist=True), A.frozen(name), name + " after refused calls")
    finally:
        h.close()
    h = _lib.Handle(0)
    try:
        with pytest.raises(ValueError, match="cc_set_params has not been called"):
            h.assign(X)
        h.points_upload(X)
        with pytest.raises(ValueError, match="cc_set_params has not been called"):   # the existing error of the online phase
            h.online_run()
    finally:
        h.close()


def test_python_face():
    """HDDStream.assign / assign_clusters on a fitted model: fresh oracles built from the model's own lists answer for 200
    held-out points; assign_clusters is the numpy join of those answers; final_clusters is untouched."""
    import scenarios as S
    from chronoclust_amd import _lib, multi
    from chronoclust_amd.clustering.hddstream import HDDStream
    n, d = 3000, 5
    data = S.make_blobs(5, n + 200, d, 12, sigma=0.02)
    fit, held = data[:n], np.ascontiguousarray(data[n:])
    # a few events far outside the box: a microcluster of a few hundred points absorbs anything inside it (one more point
    # hardly moves its radius), these would found microclusters of their own
    held[::10] = np.random.default_rng(6).uniform(3.0, 4.0, (20, d))
    m = HDDStream(S.params_to_config(S.blob_params(n, param_epsilon=0.06)))
    m.online_microcluster_maintenance(fit, 0)
    clusters_before = [(c.cumulative_weight, np.asarray(c.cluster_centroids).tobytes(), list(c.members_in_merge_order))
                       for c in m.final_clusters]
    objects_before = list(m.final_clusters)
    par = T.Params(m.epsilon_squared, m.delta_squared, m.k, m.beta, float(m.mu), float(m.omicron), m.upsilon,
                   m.upsilon ** 2, m.delta, int(m.pi))
    tables = [T.Table.__new__(T.Table) for _ in range(2)]
    for t, kind in zip(tables, (_lib.PCORE, _lib.OUTLIER)):
        t.__dict__.update(m.table(kind))
    assert len(tables[0]) > 0 and len(clusters_before) > 0
    exp = A.frozen_answers(tables[0], tables[1] if len(tables[1]) else None, par, held)
    uid, path = m.assign(held)
    A.same_assign((uid, path, None), exp, "HDDStream.assign")
    assert (path == 0).any() and (path == 2).any()
    idx = m.assign_clusters(held)
    mem, off = m._cl_arrays[0], m._cl_arrays[1]
    want = multi.point_cluster_index(np.where(exp[1] == 0, exp[0], -1), tables[0].id, tables[0].uid, mem, off)
    assert np.array_equal(idx, want) and (idx >= 0).any() and (idx[path != 0] == -1).all()
    assert all(a is b for a, b in zip(objects_before, m.final_clusters)) and len(objects_before) == len(m.final_clusters)
    assert clusters_before == [(c.cumulative_weight, np.asarray(c.cluster_centroids).tobytes(), list(c.members_in_merge_order))
                               for c in m.final_clusters]


def test_in_a_group_of_two():
    """Each rank of an in-process group assigns its own half of the points against its own replica of the table: the
    single-handle answers, and no collective is counted."""
    name = "lattice-129+64x13"
    pcores, outliers, par, X = A.case(name)[:4]
    exp = A.frozen(name)
    half = len(X) // 2
    parts = [slice(0, half), slice(half, None)]

    def work(h, rank):
        T.fill_handle(h, par, pcores, outliers)
        return h.assign(X[parts[rank]], want_dist=True)

    hs, got = T._run_group(2, work)
    try:
        for rank in range(2):
            A.same_assign(got[rank], tuple(e[parts[rank]] for e in exp), "%s rank %d of 2" % (name, rank))
            s = hs[rank].stats()
            assert s["comm_launches"] == 0 and s["sharded_windows"] == 0, s
            assert s["assign_points"] == len(X[parts[rank]]) and hs[rank].comm_info()["world"] == 2
    finally:
        for h in hs:
            h.close()
