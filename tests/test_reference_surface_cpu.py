"""Pins the CPU oracle (oracle/chrono_oracle.c) to the Python reference at the designed edges: the goldens of
tests/golden/surface/ (tests/golden/make_golden_surface.py; format and cases in tests/surface_util.py) are what the
reference computes for the streams of test_fuzz_parity and test_sequential's k_seq_r fuzz, for the decay boundary on the
lists of test_boundary_tables, for the offline phase on the small tables of table_util.OFFLINE_TABLES and for the online
phase on the small tables of table_util.ONLINE_TABLES.  Every case runs through OracleHDDStream, make_oracle and
co_decay_downgrade and must equal the recorded reference bit for bit: labels, paths, ids, weights, counters and derived
parameters value by value, the wide float columns by the SHA-256 of their bytes.  A failure names case, call and column.

The recorded set must not be trivial, and the structure a table case exists for must be present in the REFERENCE's result
(table_util.check_structure, check_online): both are asserted on the goldens alone.  Needs neither GPU nor reference."""
import numpy as np
import pytest

import surface_util as S
import table_util as T
from oracle import oracle as O

STREAM_FIELDS = ["params", "xsha", "labels_uid", "labels_path"] + S.LISTS + S.CLUSTERS
F = 2.0 ** -1.0


def test_every_set_is_recorded_as_selected():
    fuzz, left_out, seqr = S.stream_selection()
    assert S.cases_of("streams_fuzz") == ["fuzz-%d" % s for s in fuzz]
    assert S.cases_of("streams_seqr") == ["seqr-%d" % s for s in seqr]
    for meta in S.load_set("streams_fuzz")[2]:
        assert meta["left_out"] == left_out and meta["fuzz_max_points"] == S.FUZZ_MAX_POINTS
    dims = S.stream_dims()
    assert dims == {c: S.stream_case(c)[1][0].shape[1] for c in S.cases_of("streams_")}
    assert S.cases_of("boundary") == list(S.boundary_cases())
    assert S.cases_of("offline") == S.offline_cases() and len(S.offline_cases()) == 9
    assert S.cases_of("online") == S.online_cases()
    assert [n for n in S.online_cases() if "set-params" in n] == ["victims-set-params-200x20", "victims-set-params-k3-100x14"]


@pytest.mark.parametrize("case", S.cases_of("streams_"))
def test_stream_oracle_matches_reference(case):
    cfg, Xs = S.stream_case(case)
    golden = S.calls_of("streams_", case)
    assert len(golden) == len(Xs)
    S.check_inputs(case, Xs, golden)
    o = O.OracleHDDStream(cfg)
    for t, X in enumerate(Xs):
        o.online_microcluster_maintenance(X, t)
        got = S.make_record(params=(o.pi, o.mu, o.omicron) + o.counters, X=X, uid=o.labels_uid, path=o.paths,
                            tables=(o.table(O.PCORE), o.table(O.OUTLIER)), clusters=o.clusters)
        S.same_record(got, golden[t], STREAM_FIELDS, "%s timepoint %d (oracle)" % (case, t))


def test_recorded_streams_are_not_trivial():
    """Conditions on the recorded reference outputs of the test_fuzz_parity streams (the value lists are _case's)."""
    cases = S.cases_of("streams_fuzz")
    seen = {}
    first_300 = many_mcs = merged = lost = 0
    for case in cases:
        cfg, Xs = S.stream_case(case)
        d = Xs[0].shape[1]
        forms = {"0": 0, "1": 1, "d-1": max(1, d - 1), "d": d, "d+3": d + 3}
        for key in ("k", "delta", "lambda"):
            seen[(key, cfg[key])] = seen.get((key, cfg[key]), 0) + 1
        seen[("d", d)] = seen.get(("d", d), 0) + 1
        for form, value in forms.items():     # (d <= 2 makes some forms coincide: such a stream counts for none of them)
            if cfg["pi"] == value and list(forms.values()).count(value) == 1:
                seen[("pi", form)] = seen.get(("pi", form), 0) + 1
        golden = S.calls_of("streams_fuzz", case)
        first_300 += len(golden[0]["labels_uid"]) >= 300
        many_mcs += len(golden[-1]["pcore_id"]) + len(golden[-1]["outlier_id"]) >= 10
        merged += bool((np.diff(golden[-1]["cl_offsets"]) > 1).any())
        lost += any(len(set(a["outlier_uid"].tolist()) - set(b["outlier_uid"].tolist()) - set(b["pcore_uid"].tolist())) > 0
                    for a, b in zip(golden, golden[1:]))
    want = ([("k", v) for v in (0.5, 1.0, 2.0, 3.0, 4.0, 16.0, 40.0)] + [("delta", v) for v in (0.0, 0.01, 0.05, 0.3, 1.0)]
            + [("lambda", v) for v in (0.0, 0.5, 2.0, 5.0)] + [("d", v) for v in (1, 2, 3, 4, 5, 8, 9, 17, 20, 33, 64)]
            + [("pi", v) for v in ("0", "1", "d-1", "d", "d+3")])
    for key in want:
        assert seen.get(key, 0) >= 8, "%s = %s in %d recorded streams" % (key[0], key[1], seen.get(key, 0))
    assert first_300 >= 60, "%d streams start with 300 points or more" % first_300
    assert many_mcs >= 20, "%d streams end with ten microclusters or more" % many_mcs
    assert merged >= 10, "%d streams end with a cluster of several members" % merged
    assert lost >= 10, "%d streams lose an outlier microcluster between two timepoints" % lost


@pytest.mark.parametrize("case", S.cases_of("boundary"))
def test_boundary_oracle_matches_reference(case):
    pcores, outliers, par = S.boundary_case(case)
    golden = S.calls_of("boundary", case)
    o = T.make_oracle(par, pcores, outliers)
    for call, exp in enumerate(golden):
        T.oracle_lib().co_decay_downgrade(o._h, F)
        got = S.make_record(tables=(o.table(O.PCORE), o.table(O.OUTLIER)))
        S.same_record(got, exp, S.LISTS, "%s call %d (oracle)" % (case, call + 1))
    if case.startswith("flagged"):
        assert len(golden) >= 3 and len(golden[-1]["pcore_id"]) + len(golden[-1]["outlier_id"]) == 0


def test_boundary_structure_is_in_the_reference_result():
    """What test_decay_downgrade_against_oracle asserts on the oracle's lists, on the reference's: weights exactly on
    beta * mu (kept) and on omicron (deleted - or skipped by the walk), flagged pcores that the walk skipped."""
    from test_boundary_tables import BETA, MU, OMICRON
    for case in S.cases_of("boundary"):
        _, m_p, m_o, d, flagged = S.boundary_cases()[case]
        pcores, outliers, par = S.boundary_case(case)
        after = S.calls_of("boundary", case)[0]
        if flagged:                                   # every second row of a list survives a call
            assert len(after["pcore_id"]) == m_p // 2, case
            continue
        if m_p >= 100:
            w = after["pcore_w"]
            assert (w == BETA * MU).any() and (w < BETA * MU).any(), case
            gone = set(pcores.uid.tolist()) - set(after["pcore_uid"].tolist()) - set(after["outlier_uid"].tolist())
            assert len(gone) > 0, case
        if m_o >= 100:
            w = after["outlier_w"]
            assert (outliers.w * F == OMICRON).any() and (w <= OMICRON).any(), case
            assert (w == OMICRON * (1.0 + 2.0 ** -52)).any(), case


@pytest.mark.parametrize("case", S.cases_of("offline"))
def test_offline_oracle_matches_reference(case):
    t, par, meta = T.build_table(case)
    exp = S.calls_of("offline", case)[0]
    o = T.make_oracle(par, t)
    info, clusters = T.oracle_offline(o)
    got = S.make_record(tables=(o.table(O.PCORE), o.table(O.OUTLIER)), clusters=clusters, info=info)
    S.same_record(got, exp, S.LISTS + S.CLUSTERS + S.OFFLINE_INFO, "%s (oracle)" % case)
    T.check_structure(t, par, meta, S.info_of(exp), S.clusters_of(exp))      # on the reference's result


_online = {}


def online_case(name):
    if name not in _online:
        _online[name] = T.build_online(name)
    return _online[name]


def reference_online_result(case, golden):
    """What table_util.oracle_online returns, from the goldens: uid and path per point, the first call's, the pcore list
    between the two calls."""
    d = case[3].shape[1]
    res = dict(uid=golden[-1]["labels_uid"], path=golden[-1]["labels_path"])
    if len(golden) == 2:
        res["first"] = (golden[0]["labels_uid"], golden[0]["labels_path"])
        res["mid"] = dict(S.table_of(golden[0], "pcore"), pref=golden[0]["mid_pref"].reshape(-1, d))
    return res


@pytest.mark.parametrize("name", S.cases_of("online"))
def test_online_oracle_matches_reference(name):
    case = online_case(name)
    par, X, meta = case[2], case[3], case[4]
    golden = S.calls_of("online", name)
    assert len(golden) == (2 if "first" in meta else 1)
    res = T.oracle_online(case)
    o = res["o"]
    if "first" in meta:
        S.check_inputs(name, [meta["first"][1], X], golden)
        mid = res["mid"]
        got = S.make_record(uid=res["first"][0], path=res["first"][1], tables=(mid, mid), mid_pref=mid["pref"])
        S.same_record(got, golden[0], ["labels_uid", "labels_path", "mid_pref"] + [f for f in S.LISTS if f.startswith("pcore")],
                      "%s first call (oracle)" % name)
    else:
        S.check_inputs(name, [X], golden)
    got = S.make_record(params=(par.pi, par.mu, par.omicron) + o.counters, uid=res["uid"], path=res["path"],
                        tables=(o.table(O.PCORE), o.table(O.OUTLIER)))
    S.same_record(got, golden[-1], ["params", "labels_uid", "labels_path"] + S.LISTS, "%s (oracle)" % name)
    T.check_online(case, reference_online_result(case, golden))               # on the reference's result
