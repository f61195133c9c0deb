"""The validation rounds of the online phase (cc_validate.h: k_dseed, k_decide, k_claims, k_claims_heavy, k_chain, k_chain_long
plain / PREP / SPLIT, k_commit_a / b, the carry set) against the CPU oracle on DESIGNED ARRIVALS (tests/arrival_util.py): row
sequences that are periodic with the configured window, so that every full window validates exactly the designed chain lengths
- 1, the member list's 31 .. 34, k_chain_long's batch K(d) - 1 .. K(d) + 1, 2 K, 2 K + 1, its queue's 2 047 .. 2 049, 8 191 ..
8 193 in a window of 16 384 and the 49 152 claimants of one row that are the largest window -, members exactly W / L apart, in
bursts, head+tail, the whole call sorted by row, and shuffled as the control; rejected steps (breathing rows), promotions with
points that change their row at that step, and rows created inside the window, each on a chosen step of its chain.

k_dseed's lookups assume members "spread like arrivals" (gap = B / n, a backward read of 16 gaps, a walk of 64 steps): sorted
files, bursts and strict round-robin break that, and what then has to hold is the chain of fallbacks - lv = -2, lk_ok = false,
CC_T_UNKNOWN, the window commits up to that point, and at least its first one.

Every case runs under the library's own policy, with the sequential kernels forbidden and forced, with each knob that takes a
validation kernel out, and with a quarter of the window and three lookahead scans (the carry set meets the same chains).  uid
and path per point, both lists and the id counters are compared for bit equality; cc_stats says which kernels ran.

No case runs in a group of ranks.  On ordered arrivals the device counters the window policy reads (windows, truncated windows,
dirty tiles, long chains) differ from run to run on ONE handle - the member lists are unordered, and which lookups of k_dseed
succeed depends on which 32 members a list holds (profiles/arrival_orders.txt) -, so two ranks can take different decisions and
one waits for a collective the other never enters: `lens-sorted-d6-large` did in a group of two.  DESIGN.md section 2.1 states
the assumption; until the ranks agree on those counters a group test of these cases would be a test of luck.

cc_stats counts `long_chains` where k_decide's atomics or k_claims_heavy find a member list full - on the tables k_claims does
not serve (beyond 1 024 rows, or CHRONOCLUST_HIP_CLAIMS=0).  On a small table k_claims leaves the count in the row's word and
no statistic; there the prepared chains (`long_prepared`, tables of up to 64 rows) are the evidence that k_chain_long ran."""
import time

import pytest

import arrival_util as A
import table_util as T
from test_pruned_scan import _env

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

# name -> (environment around the handle's creation, set_tuning but for the window).  Every mode but the first and
# sequential2 keeps the stream on the windows (sequential=1), so that the kernels the knob selects really run.
MODES = {
    "default": ({}, {}),
    "sequential1": ({}, dict(sequential=1)),
    "sequential2": ({}, dict(sequential=2)),
    "longchains0": (dict(CHRONOCLUST_HIP_LONGCHAINS=0), dict(sequential=1)),
    "longprep0": (dict(CHRONOCLUST_HIP_LONGPREP=0), dict(sequential=1)),
    "heavy0": (dict(CHRONOCLUST_HIP_HEAVY=0), dict(sequential=1)),
    "claims0": (dict(CHRONOCLUST_HIP_CLAIMS=0), dict(sequential=1)),
    "quiet0": (dict(CHRONOCLUST_HIP_QUIET=0), dict(sequential=1)),
    "nodirty0": (dict(CHRONOCLUST_HIP_NODIRTY=0), dict(sequential=1)),
    "link0": (dict(CHRONOCLUST_HIP_LINK=0), dict(sequential=1)),
    "decide-group32": (dict(CHRONOCLUST_HIP_DECIDE_GROUP=32), dict(sequential=1)),
    "quarter-window-lookahead3": ({}, dict(lookahead=3, sequential=1)),
}
LARGE_WINDOW_MODES = ("default", "sequential1", "longchains0")

_cases = {}


def _case(name):
    """(case, oracle result) of a case, the structure check done; generator and oracle run once per case."""
    if name not in _cases:
        case = A.build_arrivals(name)
        t0 = time.time()
        exp = T.oracle_online(case)
        print("%s: oracle %.2f s" % (name, time.time() - t0))
        T.check_online(case, exp)
        _cases[name] = (case, exp)
    return _cases[name]


def _tuning(case, mode):
    """The mode's tuning with the case's window.  A large table under a knob mode syncs every two windows: what the host saw of
    long chains and heavy rows in one batch selects the listed k_chain_long and k_claims_heavy for the next, and with the
    library's own four windows to the first batch the three periods of a case would be over before either ran."""
    meta = case[4]
    t = dict(MODES[mode][1], window=meta["W"] // 4 if mode == "quarter-window-lookahead3" else meta["W"])
    if meta["large"] and mode != "default":
        t["windows_per_sync"] = 2
    return t


def _handle(case, mode):
    from chronoclust_amd import _lib
    with _env(**MODES[mode][0]):
        h = _lib.Handle(0)
    h.set_tuning(**_tuning(case, mode))
    return h


def check_stats(case, mode, s):
    """What cc_stats can tell about the kernels that ran."""
    meta = case[4]
    assert s["points"] == len(case[3])
    if mode == "sequential2":
        assert s["seq_points"] > 0, s
        return
    if mode == "default":
        assert s["windows"] > 0 or s["seq_points"] > 0, s
        return
    assert s["seq_points"] == 0 and s["seq_r_points"] == 0 and s["seq_g_points"] == 0 and s["windows"] > 0, s
    full = mode != "quarter-window-lookahead3"
    longest = meta["longest"] if full else meta["longest"] // 4
    if mode == "quarter-window-lookahead3":
        assert s["windows"] >= len(case[3]) // (meta["W"] // 4), s
    if longest > 40 and (meta["large"] or mode == "claims0"):     # the tables whose long chains are counted (see above)
        assert s["long_chains"] > 0, s
    if mode == "longchains0":
        assert s["long_chain_launches"] == 0 and s["long_prepared"] == 0, s
    if mode == "longprep0":
        assert s["long_prepared"] == 0, s
    if meta["breathing"] and full and not meta["large"] and mode not in ("longchains0", "longprep0", "claims0"):
        assert s["long_prepared"] > 0 and 0 < s["long_replayed"], s   # a table of up to 64 rows: every long pcore chain prepared
    if meta["large"] and longest > 40:
        assert (s["heavy_launches"] > 0) == (mode != "heavy0"), s     # from the second batch on: the third period
        assert (s["long_chain_launches"] > 0) == (mode != "longchains0"), s
    else:
        assert s["heavy_launches"] == 0 or mode == "claims0", s


@pytest.mark.parametrize("name,mode", [(n, m) for n in A.W4096 for m in MODES])
def test_arrivals_against_oracle(name, mode):
    case, exp = _case(name)
    h = _handle(case, mode)
    try:
        T.same_online(h, T.handle_online(h, case), exp, "%s [%s]" % (name, mode))
        s = h.stats()
        print("%s [%s]: run %.2f ms, %d windows, %d truncated, %d rounds, long %d / %d prepared %d replayed %d heavy %d" % (
            name, mode, s["run_ms"], s["windows"], s["truncated"], s["rounds"], s["long_chains"], s["long_chain_launches"],
            s["long_prepared"], s["long_replayed"], s["heavy_launches"]))
        check_stats(case, mode, s)
    finally:
        h.close()


@pytest.mark.timeout(300)   # one chain of 49 152 steps per window and round at k_chain's 0.5 - 2 us a step: 0.1 s a round, 8 rounds, 3 windows
@pytest.mark.parametrize("name,mode", [(n, m) for n in A.LARGE_WINDOW for m in LARGE_WINDOW_MODES])
def test_arrivals_in_large_windows_against_oracle(name, mode):
    """Windows of 16 384 (chains of 8 191 .. 8 193) and of 49 152, every point of which is one row's."""
    case, exp = _case(name)
    h = _handle(case, mode)
    try:
        T.same_online(h, T.handle_online(h, case), exp, "%s [%s]" % (name, mode))
        check_stats(case, mode, h.stats())
    finally:
        h.close()
