"""The kernels against the Python reference at the designed edges: the goldens of tests/golden/surface/
(tests/golden/make_golden_surface.py; format and cases in tests/surface_util.py), compared directly - the oracle is never
called here.  test_reference_surface_cpu.py holds the oracle against the same goldens; the tests that compare the kernels
with the oracle (test_fuzz_parity, test_sequential, test_pruned_scan, test_boundary_tables, test_offline_tables,
test_online_tables) cover more code paths per case and name the differing element.

Streams (test_fuzz_parity._case, test_sequential._seq_r_case) run through HDDStream with the library's defaults, with the
sequential kernels forced and - from nine dimensions on, where a pruned chain exists - with pruned scans forced on the
windows.  The tables go into a handle by table_util.fill_handle: the decay boundary twice (the all-flagged lists until they
are empty), the offline phase on one GPU, the online phase under the modes default, prune2 and sequential2 of
test_online_tables.  Labels, paths, ids, weights, counters and derived parameters are compared value by value, the wide
float columns by the SHA-256 of their bytes; a failure names case, call and column."""
import pytest

import surface_util as S
import table_util as T
from test_online_tables import MODES, _handle, _modes_of
from test_pruned_scan import _env

pytestmark = pytest.mark.gpu

STREAM_FIELDS = ["params", "xsha", "labels_uid", "labels_path"] + S.LISTS + S.CLUSTERS
F = 2.0 ** -1.0

# name -> (environment around the handle's creation, tuning)
STREAM_MODES = {
    "default": ({}, None),
    "sequential2": ({}, dict(sequential=2)),
    "prune2": (dict(CHRONOCLUST_HIP_PRUNE=2), dict(sequential=1)),
    "seq_r": ({}, dict(window=1024, sequential=2)),     # test_register_resident_sequential_kernel_fuzz's tuning
}


def _stream_modes(case, d):
    if case.startswith("seqr"):
        return ["default", "seq_r"]
    return ["default", "sequential2"] + (["prune2"] if d >= 9 else [])


def _hdd_record(h, X):
    clusters = [dict(members=c.members_in_merge_order, w=c.cumulative_weight, cf1=c.CF1, cf2=c.CF2,
                     cen=c.cluster_centroids, pref=c.preferred_dimension_vector) for c in h.final_clusters]
    return S.make_record(params=(h.pi, h.mu, h.omicron, h.pcore_MC_last_id, h.outlier_MC_last_id), X=X, uid=h.labels_uid,
                         path=h.labels_path, tables=(h.table(0), h.table(1)), clusters=clusters)


@pytest.mark.parametrize("case,mode", [(c, m) for c, d in S.stream_dims().items() for m in _stream_modes(c, d)])
def test_stream_matches_reference(case, mode):
    from chronoclust_amd.clustering.hddstream import HDDStream
    cfg, Xs = S.stream_case(case)
    golden = S.calls_of("streams_", case)
    assert len(golden) == len(Xs)
    S.check_inputs(case, Xs, golden)
    env, tuning = STREAM_MODES[mode]
    with _env(**env):                                   # (the knob is read when the handle is created)
        h = HDDStream(cfg, tuning=tuning)
    seq_r = 0
    for t, X in enumerate(Xs):
        h.online_microcluster_maintenance(X, t)
        S.same_record(_hdd_record(h, X), golden[t], STREAM_FIELDS, "%s timepoint %d [%s]" % (case, t, mode))
        seq_r += h.stats()["seq_r_points"]
    if mode == "seq_r":
        assert seq_r > 0


def _handle_lists(h):
    return h.export(0), h.export(1)


@pytest.mark.parametrize("case", S.cases_of("boundary"))
def test_boundary_matches_reference(case):
    from chronoclust_amd import _lib
    pcores, outliers, par = S.boundary_case(case)
    golden = S.calls_of("boundary", case)
    assert len(golden) >= 2
    h = T.fill_handle(_lib.Handle(0), par, pcores, outliers)
    try:
        for call, exp in enumerate(golden):             # (twice; the all-flagged lists until nothing is left)
            h.decay_downgrade(F)
            S.same_record(S.make_record(tables=_handle_lists(h)), exp, S.LISTS, "%s call %d" % (case, call + 1))
    finally:
        h.close()


@pytest.mark.parametrize("case", S.cases_of("offline"))
def test_offline_matches_reference(case):
    from chronoclust_amd import _lib
    t, par, _ = T.build_table(case)
    exp = S.calls_of("offline", case)[0]
    h = _lib.Handle(0)
    try:
        info, clusters = T.handle_offline(T.fill_handle(h, par, t))
        got = S.make_record(tables=_handle_lists(h), clusters=clusters, info=info)
        S.same_record(got, exp, S.LISTS + S.CLUSTERS + S.OFFLINE_INFO, case)
    finally:
        h.close()


_online = {}


def _online_case(name):
    if name not in _online:
        _online[name] = T.build_online(name)
    return _online[name]


@pytest.mark.parametrize("name,mode", [(n, m) for n in S.cases_of("online") for m in _modes_of(n)
                                       if m in ("default", "prune2", "sequential2")])
def test_online_matches_reference(name, mode):
    pcores, outliers, par, X, meta = _online_case(name)
    golden = S.calls_of("online", name)
    assert len(golden) == (2 if "first" in meta else 1)
    what = "%s [%s]" % (name, mode)
    h = _handle(*MODES[mode])
    try:
        if "first" in meta:                             # (table_util.handle_online's steps, the lists read in between)
            par0, X0 = meta["first"]
            S.check_inputs(name, [X0, X], golden)
            h.set_params(*par0)
            uid, path = h.online(X0)
            mid = _handle_lists(h)
            got = S.make_record(params=(par0.pi, par0.mu, par0.omicron) + tuple(h.counters()), uid=uid, path=path,
                                tables=mid, mid_pref=mid[0]["pref"])
            S.same_record(got, golden[0], ["params", "labels_uid", "labels_path", "mid_pref"] + S.LISTS, what + " first call")
            h.set_params(*par)
        else:
            S.check_inputs(name, [X], golden)
            T.fill_handle(h, par, pcores, outliers)
        uid, path = h.online(X)
        got = S.make_record(params=(par.pi, par.mu, par.omicron) + tuple(h.counters()), uid=uid, path=path,
                            tables=_handle_lists(h))
        S.same_record(got, golden[-1], ["params", "labels_uid", "labels_path"] + S.LISTS, what)
    finally:
        h.close()
