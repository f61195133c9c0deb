"""The sequential kernels of the online phase - k_seq_r (table in registers, d = 2 .. 4), k_seq (table in LDS), k_seq_g (table in HBM,
narrow up to 128 dimensions, wide up to 1 024) - and the hand-over between them (OnlineRun::sequential_stint, SeqHandover) against the
CPU oracle on inputs designed for THEIR constants (tests/seq_edge_util.py): k_seq_r's 64 pcore slots and 64 QO outlier slots reached
by promotion and by creation on chosen points of a chunk, slots burnt by promotions and given back by the reload every 8 192 points,
ties across lanes, slots and the `n_lanes <= 16` shortcut; k_seq's image of 6600 / (4 d + 5) rows filled on the last point of a
staged chunk and found full on the first of another, in all four <FILTER, POW2> instances; k_seq_g's rows q and q + 1 024 of one
thread, its wave boundaries, every width at which its chunk or its form changes, one point per chunk.

Every case runs on a fresh handle with the sequential kernels forced (sequential=2), forced without k_seq_r (d <= 4), forced without
k_seq_g (where the table outgrows k_seq's image: the windows take the rest) and under the library's own policy.  uid and path per
point, both lists and the id counters are compared for bit equality (same_online); in the forced modes cc_stats' seq_points,
seq_r_points and seq_g_points must EQUAL what seq_edge_util.model_shares - the hand-over rules in plain Python over the oracle's
paths - says each kernel takes: a hand-over that drops or repeats a point, or stops one point early or late, fails here even where
the labels survive it.  Without k_seq_g only seq_g_points == 0 and the sequential share up to the stop are asserted.

tests/test_sequential_edges_cpu.py asserts without a GPU that every case holds its design.  The oracle is the referee: no goldens
of the Python reference accompany these cases, since it cannot be imported where the suite is built."""
import time

import pytest

import seq_edge_util as S
import table_util as T
from test_pruned_scan import _env

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]

_cases = {}


def _case(name):
    """(case, oracle result) of a case, the structure check done; generator and oracle run once per case."""
    if name not in _cases:
        case = S.build_seq_edge(name)
        t0 = time.time()
        exp = T.oracle_online(case)
        print("%s: oracle %.2f s" % (name, time.time() - t0))
        T.check_online(case, exp)
        _cases[name] = (case, exp)
    return _cases[name]


def _modes(name):
    gen, kw = S.SEQ_EDGE_CASES[name]
    return S.modes_of(gen(**kw)) + ["default"]


def _run(name, mode):
    case, exp = _case(name)
    from chronoclust_amd import _lib
    with _env(**S.MODES.get(mode, {})):
        h = _lib.Handle(0)
    try:
        if mode != "default":
            h.set_tuning(sequential=2)
        t0 = time.time()
        labels = T.handle_online(h, case)
        s = h.stats()
        print("%s [%s]: %.1f ms | points %d seq %d seq_r %d seq_g %d windows %d" % (
            name, mode, 1e3 * (time.time() - t0), s["points"], s["seq_points"], s["seq_r_points"], s["seq_g_points"], s["windows"]))
        T.same_online(h, labels, exp, "%s [%s]" % (name, mode))
        assert s["points"] == len(case[3])
        if mode == "default":
            return
        want = S.model_shares(case, exp["path"], S.MODES[mode])
        assert want == case[4]["shares"][mode], "the model and the design disagree (tests/test_sequential_edges_cpu.py)"
        got = {k: s[k] for k in ("seq_points", "seq_r_points", "seq_g_points")}
        assert got == {k: want[k] for k in got}, "%s [%s]: cc_stats %r, the hand-over model %r" % (name, mode, got, want)
        assert (s["windows"] > 0) == (want["window_points"] > 0), s
    finally:
        h.close()


@pytest.mark.parametrize("name,mode", [(n, m) for n in S.SEQ_EDGE_CASES for m in _modes(n)])
def test_sequential_edge_against_oracle(name, mode):
    _run(name, mode)
