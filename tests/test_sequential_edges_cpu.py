"""The designed inputs of tests/test_sequential_edges.py against the CPU oracle alone (no GPU): every case of
seq_edge_util.SEQ_EDGE_CASES is built, the oracle runs the online phase on it, and `check_online` asserts that the case holds its
design - uid and path of every point as written, every promotion and creation at its index with the list sizes before and after,
the tied rows at bit-equal distances and the smallest key the winner.  The hand-over model's shares are held against the figures
written down HERE, case by case, from the kernels' constants: a generator changed so that an event moves by one point fails.  The
constants themselves are held against the source lines that define them.

No goldens of the Python reference: it cannot be imported where this suite is built; the oracle is the referee."""
import os
import re

import numpy as np
import pytest

import seq_edge_util as S
import table_util as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_results = {}


def _case(name):
    if name not in _results:
        case = S.build_seq_edge(name)
        _results[name] = (case, T.oracle_online(case))
    return _results[name]


def _src(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_constants_are_the_kernels():
    """The capacities, chunks and stop tests the cases sit on, as the source states them."""
    seq_r, seq, seq_g = (_src("chronoclust_amd", "csrc", f) for f in ("cc_seq_r.h", "cc_seq.h", "cc_seq_g.h"))
    host, run, api = _src("chronoclust_amd", "csrc", "cc_host.h"), _src("chronoclust_amd", "csrc", "cc_online_run.h"), \
        _src("include", "chronoclust_hip.h")
    assert "static constexpr int QO = D <= 3 ? 4 : 3;" in seq_r
    assert "bool fits = M <= 64 + 64 * QO;" in seq_r and "fits = n_p <= 64 && n_o <= 64 * QO;" in seq_r
    assert "if (n_p >= 64 || n_os >= 64 * QO) { full = true; break; }" in seq_r
    assert "if (n_lanes <= 16) return a;" in seq_r
    assert "ctl->seq_rest = n - done;" in seq_r
    assert int(re.search(r"^#define CC_SEQ_DOUBLES (\d+)", host, re.M).group(1)) == S.SEQ_DOUBLES
    assert "return CC_SEQ_DOUBLES / (4 * d + 5);" in host
    assert [S.seq_cap_rows(d) for d in (2, 3, 4, 5, 8, 13, 20, 40, 64)] == [507, 388, 314, 264, 178, 115, 77, 40, 25]
    assert int(re.search(r"^#define CC_SEQ_CHUNK_DOUBLES (\d+)", seq, re.M).group(1)) == 512
    assert "const int C = (CC_SEQ_CHUNK_DOUBLES / d) < 64 ? (CC_SEQ_CHUNK_DOUBLES / d) : 64;" in seq
    assert "if (M >= cap) { full = true; break; }" in seq
    assert [S.seq_chunk(d) for d in (5, 8, 13, 20, 40, 64)] == [64, 64, 39, 25, 12, 8]
    for name, want in (("CC_SEQG_THREADS", "1024"), ("CC_SEQG_CHUNK_DOUBLES", "512"), ("CC_SEQG_NARROW_DIM", "128"),
                       ("CC_SEQG_WIDE_DOUBLES", "CC_MAX_DIM")):
        assert re.search(r"^#define %s (\w+)" % name, seq_g, re.M).group(1) == want, name
    assert int(re.search(r"^#define CC_MAX_DIM (\d+)", api, re.M).group(1)) == 1024
    assert int(re.search(r"^#define CC_WINDOW_MAX_DIM (\d+)", api, re.M).group(1)) == S.WINDOW_MAX_DIM
    assert [S.seq_g_chunk(d) for d in (65, 127, 128, 129, 191, 192, 193, 512, 513, 1024)] == [7, 4, 4, 7, 5, 5, 5, 2, 1, 1]
    assert "const int chunk = %d;" % S.HOST_CHUNK in run
    assert "seq.on() ? %d : 0" % S.HOST_CHUNK in run


@pytest.mark.parametrize("name", list(S.SEQ_EDGE_CASES))
def test_case_holds_its_design(name):
    case, res = _case(name)
    T.check_online(case, res)


@pytest.mark.parametrize("name", list(S.SEQ_EDGE_CASES))
def test_model_gives_the_designed_shares(name):
    """model_shares over the oracle's paths against the shares the generator wrote from its event indices, mode by mode."""
    case, res = _case(name)
    n = len(case[3])
    modes = S.modes_of(case)
    assert "seq2" in modes and ("seq2-seqr0" in modes) == (case[3].shape[1] <= 4)
    for mode in modes:
        got = S.model_shares(case, res["path"], S.MODES[mode])
        assert got == case[4]["shares"][mode], (name, mode)
        assert got["seq_points"] + got["window_points"] == n and got["seq_r_points"] + got["seq_g_points"] <= got["seq_points"]


# (points, k_seq_r's points, the point at which the LDS kernels stop - None: they never do) with sequential=2, written from the
# kernels' constants: r-p63-atJ J + 1; r-o-fill five promotions + two creations; r-l-g 2 creations to 192 slots, 64 to 314 rows
# at a creation every other point; l-cap 2 C (slack 1: C) with C = min(64, 512 / d)
EXPECTED = {
    "r-lanes16-d2": (8196, 8196, None), "r-lanes16-d3": (8196, 8196, None), "r-lanes16-d4": (8196, 8196, None),
    "r-p63-at0-d3": (30, 1, None), "r-p63-at63-d3": (93, 64, None), "r-p63-at64-d3": (94, 65, None),
    "r-p63-at100-d3": (130, 101, None), "r-p63-at63-d2": (93, 64, None), "r-p63-at63-d4": (93, 64, None),
    "r-p64-d3": (35, 0, None), "r-p65-d3": (35, 0, None),
    "r-o-fill-d3": (13, 7, None), "r-o-fill-d4": (13, 7, None), "r-o-full-d2": (9, 0, None), "r-o-over-d4": (9, 0, None),
    "r-slot-ties-d3": (20, 20, None), "r-reload-d3": (8257, 8257, None), "r-l-g-d4": (140, 3, 128),
    "l-cap-d5": (193, 0, 128), "l-cap-d8": (193, 0, 128), "l-cap-d13": (118, 0, 78), "l-cap-d20": (76, 0, 50),
    "l-cap-d40": (37, 0, 24), "l-cap-d64": (25, 0, 16), "l-cap-1-d20": (76, 0, 25), "l-cap-0-d20": (76, 0, 0),
}


@pytest.mark.parametrize("name", list(EXPECTED))
def test_shares_are_the_intended_ones(name):
    case, res = _case(name)
    n, r, stop = EXPECTED[name]
    d = case[3].shape[1]
    assert len(case[3]) == n
    full = S.model_shares(case, res["path"], {})
    assert full["seq_points"] == n and full["seq_r_points"] == r and full["window_points"] == 0
    assert full["seq_g_points"] == (0 if stop is None else n - stop)
    if d <= 4:
        no_r = S.model_shares(case, res["path"], dict(CHRONOCLUST_HIP_SEQR=0))
        assert no_r == dict(full, seq_r_points=0)
    no_g = S.model_shares(case, res["path"], dict(CHRONOCLUST_HIP_SEQG=0))
    assert no_g["seq_g_points"] == 0 and no_g["seq_points"] == (n if stop is None else stop)
    assert no_g["window_points"] == n - no_g["seq_points"] and no_g["seq_r_points"] == min(r, no_g["seq_points"])


def _events(case, what):
    return [e for e in case[4]["events"] if e["what"] == what]


def test_register_kernel_events_sit_on_its_capacities():
    for d in (2, 3, 4):
        case, res = _case("r-lanes16-d%d" % d)
        meta = case[4]
        e = [e for e in meta["events"] if e["at"] == meta["pcore17_at"]][0]
        assert e["what"] == "promotion" and e["n_p"] == (16, 17)
        first, second, third = meta["ties"][0], meta["ties"][1], meta["ties"][2]
        assert first["at"] < e["at"] and first["absorbed"]                              # 16 lanes: tied, absorbed
        assert second["at"] == e["at"] and not second["absorbed"] and second["win_w"] == 7.0 and second["lose_w"] == [15.0]
        assert third["at"] > e["at"] and len(meta["ties"]) == 5
        assert meta["reload_tie_at"] >= S.HOST_CHUNK and meta["ties"][4]["at"] == meta["reload_tie_at"]
        prom = _events(case, "promotion")
        rows = {int(u): i for i, u in enumerate(case[1].uid)}
        a, b = prom[1], prom[2]                                                          # promoted against their row order
        assert a["at"] < b["at"] < S.HOST_CHUNK and rows[a["uid"]] > rows[b["uid"]] and meta["ties"][4]["winner"] == a["uid"]
    for name, at in (("r-p63-at0-d3", 0), ("r-p63-at63-d3", 63), ("r-p63-at64-d3", 64), ("r-p63-at100-d3", 100),
                     ("r-p63-at63-d2", 63), ("r-p63-at63-d4", 63)):
        case, res = _case(name)
        e = [e for e in case[4]["events"] if e["n_p"] == (63, 64)]
        assert len(e) == 1 and e[0]["at"] == at and res["path"][at] == 5
        later = [x["what"] for x in case[4]["events"] if x["at"] > at]
        assert "promotion" in later and "creation" in later                              # numbered behind the stop, by k_seq
    for name, m_p in (("r-p64-d3", 64), ("r-p65-d3", 65)):
        assert len(_case(name)[0][0]) == m_p
    for d in (3, 4):
        case, res = _case("r-o-fill-d%d" % d)
        slots = 64 * S.seq_r_qo(d)
        assert len(case[1]) == slots - 2 and [e["what"] for e in case[4]["events"]][:7] == ["promotion"] * 5 + ["creation"] * 2
        assert [e["at"] for e in case[4]["events"]][:7] == list(range(7))
        assert case[4]["events"][6]["n_o"] == (slots - 6, slots - 5) and res["path"][7] == 0      # fewer outliers, every slot used
    assert len(_case("r-o-full-d2")[0][1]) == 256 and len(_case("r-o-over-d4")[0][1]) == 193
    case, res = _case("r-slot-ties-d3")
    row = {int(u): i for i, u in enumerate(case[1].uid)}
    tied = [sorted(row[u] for u, _ in t["rows"]) for t in case[4]["ties"]]
    assert [3, 67, 131] in tied and [7, 71, 135] in tied and [15, 16] in tied and [31, 32] in tied and [47, 48] in tied
    assert [18, 81] in tied and [35, 162] in tied
    paths = [int(res["path"][t["at"]]) for t in case[4]["ties"]]
    assert 1 in paths and 5 in paths                                                     # joins, and promotions out of a tie
    case, res = _case("r-reload-d3")
    before = [e for e in case[4]["events"] if e["at"] < S.HOST_CHUNK]
    assert sorted(e["what"] for e in before) == ["creation"] * 5 + ["promotion"] * 4
    assert any(e["at"] == S.HOST_CHUNK - 1 and e["what"] == "creation" for e in before)
    sixth = [e for e in case[4]["events"] if e["at"] >= S.HOST_CHUNK]
    assert len(sixth) == 1 and sixth[0]["at"] == case[4]["sixth_creation_at"] < len(case[3]) - 1
    assert len(case[1]) + 6 >= 256 and sixth[0]["n_o"] == (251, 252)                     # slots without the reload / rows with it
    case, res = _case("r-l-g-d4")
    assert len(_events(case, "creation")) == 70 and (len(case[0]), len(case[1])) == (60, 190)


@pytest.mark.parametrize("d", list(S.L_CAP_VARIANT))
def test_lds_kernel_events_sit_on_its_capacity(d):
    case, res = _case("l-cap-d%d" % d)
    cap, C = S.seq_cap_rows(d), S.seq_chunk(d)
    pcores, outliers, par, X, meta = case
    assert len(pcores) + len(outliers) == cap - 2 and len(pcores) > len(outliers)
    created = [e["at"] for e in _events(case, "creation")]
    assert created[:3] == [C - 1, C, 2 * C] and meta["stop_at"] == 2 * C
    rows_before = [len(pcores) + len(outliers) + i for i in range(3)]
    assert rows_before == [cap - 2, cap - 1, cap]
    kw = S.L_CAP_VARIANT[d]
    assert (par.pi < d) == bool(kw.get("filt")) and par.k == kw.get("k", 4.0)
    assert len(meta["ties"]) >= 3 and any(t["at"] > meta["stop_at"] for t in meta["ties"])


def test_every_filter_and_k_instance_meets_a_cap():
    seen = set()
    for d in S.L_CAP_VARIANT:
        par = _case("l-cap-d%d" % d)[0][2]
        seen.add((par.pi < d, np.frexp(par.k)[0] == 0.5))
    assert seen == {(False, True), (True, True), (False, False), (True, False)}


def test_short_calls_and_full_images():
    for d, ns in S.L_N.items():
        C = S.seq_chunk(d)
        assert ns == (1, C - 1, C, C + 1)
        for n in ns:
            case, res = _case("l-n%d-d%d" % (n, d))
            assert len(case[3]) == n and res["path"][n - 1] == 2
            assert len(case[0]) + len(case[1]) + int((res["path"] == 2).sum()) < S.seq_cap_rows(d)
    case, res = _case("l-cap-1-d20")
    assert len(case[0]) + len(case[1]) == S.seq_cap_rows(20) - 1 and [e["at"] for e in _events(case, "creation")][:2] == [24, 25]
    case, res = _case("l-cap-0-d20")
    assert len(case[0]) + len(case[1]) == S.seq_cap_rows(20)


def test_workgroup_kernel_cases():
    for d in S.G_DIMS:
        case, res = _case("g-dims-d%d" % d)
        assert (len(case[0]), len(case[1])) == (100, 64) and len(case[3]) >= 3 * S.seq_g_chunk(d) + 1
        assert S.model_shares(case, res["path"], {})["seq_g_points"] == len(case[3])
    for d in (128, 513):
        case, res = _case("g-dims-filter-d%d" % d)
        assert case[2].pi == d - 2 and case[2].k == 3.0 and len(case[3]) >= 3 * S.seq_g_chunk(d) + 1
        assert {0, 1, 2, 5} <= set(int(x) for x in res["path"]) or d == 513 and {0, 2, 5} <= set(int(x) for x in res["path"])
    for d in (20, 129):
        case, res = _case("g-stride-d%d" % d)
        assert (len(case[0]), len(case[1]), len(case[3])) == (1025, 1025, 300)
        rows = [{int(u): i for i, u in enumerate(t.uid)} for t in (case[0], case[1])]
        tied = set()
        for t in case[4]["ties"]:
            where = []
            for u, _ in t["rows"]:
                where.append(("p", rows[0][u]) if u in rows[0] else ("o", rows[1][u]))
            tied.add(tuple(sorted(where)))
        for kind in ("p", "o"):
            assert ((kind, 0), (kind, 1024)) in tied and ((kind, 1023), (kind, 1024)) in tied and ((kind, 63), (kind, 64)) in tied
        assert (("o", 500), ("p", 500)) in tied                                         # a promoted row against an older pcore
        promo = [e["at"] for e in _events(case, "promotion")]
        mixed = [t["at"] for t in case[4]["ties"] if len({u in rows[0] for u, _ in t["rows"]}) == 2]
        assert len(mixed) == 1 and (mixed[0] - 2) in promo
    for n in (1, 2):
        case, res = _case("g-one-point-d1024-n%d" % n)
        assert case[3].shape == (n, 1024) and len(case[0]) + len(case[1]) == 200 and case[4]["ties"][0]["at"] == n - 1
