"""The online phase (snapshot scans plain and pruned, k_decide / k_chain / k_commit, the sequential kernels, the split over
the ranks of a group) against the CPU oracle on INJECTED tables (tests/table_util.py, ONLINE_TABLES): tables a stream never
leaves behind - stored preference entries that disagree with the rows' variances and with the current k (`victims`, `stale`:
the handle is tainted), rows shuffled against their geometry, lattice tables on which equal distances are equal bit for bit
and thresholds are met exactly (`lattice`), more rows than points.

Every case runs through every code path the library can be put on from outside: its own policy, pruned scans forced
(CHRONOCLUST_HIP_PRUNE=2; with CHRONOCLUST_HIP_SCANP3=0 the prefix test on the VALU) and forbidden (PRUNE=0), the
sequential kernels forced and forbidden, windows of 64 points with three lookahead scans in flight (promotions and
recomputed entries change the table between the windows of one call), and in-process groups of 2 and 3 ranks with every
split forced on.  uid and path per point, both lists and the id counters are compared for bit equality; cc_stats says
which kernels ran.

A tainted handle (a stored entry may lie outside {1, k}) launches no pruned chain: `scan_p_launches == 0` whatever the
knobs say.  Phase A of k_scan_p3<GENERAL> bounds a row's distance from below with min(1, 1 / k) for the smallest weight a
dimension can have, while phase B divides by the stored entry: an entry above max(k, 1) weighs less, the bound is unsound,
and the `victims` tables are built so that the reference's nearest row is abandoned by it."""
import math
import time

import pytest

import table_util as T
from test_pruned_scan import _env

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

LARGE = ("victims-k4-10000x20", "clean-9999x20", "clean-10000x20", "clean-10001x20", "clean-19999x20", "clean-20000x20",
         "lattice-7000+3000x20")
SMALL = [n for n in T.ONLINE_TABLES if n not in LARGE]

# name -> (environment around the handle's creation, set_tuning).  The knob modes keep the stream on the windows
# (sequential=1: never hand it to a sequential kernel), so that the scans they select really run.
MODES = {
    "default": ({}, {}),
    "prune2": (dict(CHRONOCLUST_HIP_PRUNE=2), dict(sequential=1)),
    "prune0": (dict(CHRONOCLUST_HIP_PRUNE=0), dict(sequential=1)),
    "prune2-scanp3-0": (dict(CHRONOCLUST_HIP_PRUNE=2, CHRONOCLUST_HIP_SCANP3=0), dict(sequential=1)),
    "sequential1": ({}, dict(sequential=1)),
    "sequential2": ({}, dict(sequential=2)),
    "window64-lookahead3": ({}, dict(window=64, lookahead=3, sequential=1)),
}
WINDOW_MAX_DIM = 64  # beyond it the online phase is k_seq_g whatever the tuning, and no group exists

_cases = {}


def _case(name):
    """(case, oracle result) of a table, the structure check done; generator and oracle run once per table."""
    if name not in _cases:
        case = T.build_online(name)
        t0 = time.time()
        exp = T.oracle_online(case)
        print("%s: oracle %.1f s" % (name, time.time() - t0))
        T.check_online(case, exp)
        _cases[name] = (case, exp)
    return _cases[name]


def _handle(env, tuning):
    from chronoclust_amd import _lib
    with _env(**env):
        h = _lib.Handle(0)
    if tuning:
        h.set_tuning(**tuning)
    return h


def _scans(case):
    """(k_scan_u serves the plain scan, the pruned chain) as the scan plan offers them to the case: neither while the handle is
    tainted (taint clears Ctl::pow2, and with it the scalar operands and the x * (1 / k) shortcut; no chain is offered), else
    by width, filter and k."""
    from chronoclust_amd import _lib
    par, X, meta = case[2], case[3], case[4]
    d = X.shape[1]
    if meta["tainted"] or d > WINDOW_MAX_DIM:
        return False, "none"
    return _lib.scan_width(d, par.pi < d, math.frexp(par.k)[0] == 0.5)[1:]


def _chain(case):
    return _scans(case)[1]


def _check_scan_u(case, s):
    """scan_u_launches counts the windows whose plain scan is k_scan_u (pruned or not): none on a tainted handle, every
    window's on an untainted one where the width has a scalar-operand scan."""
    if case[4]["tainted"]:
        assert s["scan_u_launches"] == 0, s
    else:
        assert (s["scan_u_launches"] > 0) == (_scans(case)[0] and s["windows"] > 0), (_scans(case), s)


def _check_stats(case, mode, s):
    """What cc_stats can tell about the kernels that ran (after the case's last online call)."""
    X, meta = case[3], case[4]
    n, d = X.shape
    chain = _chain(case)
    assert s["points"] == n
    if d > WINDOW_MAX_DIM:
        assert s["seq_g_points"] == n and s["scan_u_launches"] == 0, s
        return
    _check_scan_u(case, s)
    if meta["tainted"]:
        assert s["scan_p_launches"] == 0 and s["probe_launches"] == 0, s   # no pruned chain on a tainted handle
    if mode == "prune0":
        assert s["scan_p_launches"] == 0, s
    if mode == "prune2":
        assert (s["scan_p_launches"] > 0) == (chain != "none" and s["windows"] > 0), (chain, s)
    if mode == "prune2-scanp3-0":    # (the GENERAL chain is k_scan_p3: without it plain scans)
        assert (s["scan_p_launches"] > 0) == (chain == "common" and s["windows"] > 0), (chain, s)
    if mode == "sequential2":
        assert s["seq_points"] > 0, s
    elif mode != "default":
        assert s["seq_points"] == 0 and s["seq_g_points"] == 0 and s["windows"] > 0, s
    if mode == "window64-lookahead3":
        assert s["windows"] >= (n + 63) // 64, s


def _modes_of(name):
    d = T.ONLINE_TABLES[name][1]["d"]
    return list(MODES) if d <= WINDOW_MAX_DIM else ["default", "sequential2"]


@pytest.mark.parametrize("name,mode", [(n, m) for n in SMALL for m in _modes_of(n)])
def test_online_table_against_oracle(name, mode):
    case, exp = _case(name)
    h = _handle(*MODES[mode])
    try:
        T.same_online(h, T.handle_online(h, case), exp, "%s [%s]" % (name, mode))
        _check_stats(case, mode, h.stats())
    finally:
        h.close()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", [n for n in SMALL if T.ONLINE_TABLES[n][1]["d"] <= WINDOW_MAX_DIM])
def test_online_table_in_a_group_against_oracle(name, world):
    """Rows split over the ranks from the first row (thresholds 0): every window is a sharded one, every rank holds the
    oracle's labels and lists."""
    case, exp = _case(name)
    hs, labels, stats = T.group_online(world, case)
    try:
        for rank in range(world):
            T.same_online(hs[rank], labels[rank], exp, "%s rank %d of %d" % (name, rank, world))
            s = stats[rank]
            assert s["windows"] > 0 and s["sharded_windows"] == s["windows"] and s["seq_points"] == 0, s
            _check_scan_u(case, s)
            if case[4]["tainted"]:
                assert s["scan_p_launches"] == 0, s
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize("name", ["victims-k4-600x20", "victims-filter-600x20", "clean-2000+1000x20", "lattice-1000+500x14"])
def test_online_table_in_a_group_with_pruned_scans_forced(name):
    """Two ranks, CHRONOCLUST_HIP_PRUNE=2: seeds and thresholds over all rows on every rank, phases A and B over the rank's
    own rows - where a chain exists; none on the tainted tables."""
    case, exp = _case(name)
    with _env(CHRONOCLUST_HIP_PRUNE=2):
        hs, labels, stats = T.group_online(2, case)
    try:
        for rank in range(2):
            T.same_online(hs[rank], labels[rank], exp, "%s rank %d of 2, pruning forced" % (name, rank))
            s = stats[rank]
            assert s["sharded_windows"] == s["windows"] > 0, s
            assert (s["scan_p_launches"] > 0) == (_chain(case) != "none"), s
            _check_scan_u(case, s)
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize("env", [dict(CHRONOCLUST_HIP_PRUNE=2), dict(CHRONOCLUST_HIP_PRUNE=2, CHRONOCLUST_HIP_SCANP3=0)],
                         ids=["scan_p3", "scanp3-0"])
@pytest.mark.parametrize("name", ["clean-9999x20", "clean-10000x20", "clean-10001x20", "lattice-7000+3000x20"])
def test_ten_thousand_rows_select_another_pruned_scan(name, env):
    """The common case's pruned scan of a window changes its form at 10 000 table rows (cc_stats cannot tell the forms
    apart; the table size selects them): with the library's defaults k_scan_p3 walks the rows phase A kept from per-wave
    lists (LISTED, CHRONOCLUST_HIP_P3_LISTED = 10 000) instead of testing them in place; with CHRONOCLUST_HIP_SCANP3=0
    phase A becomes a kernel of its own (k_scan_a + k_scan_p<MASKED>, CHRONOCLUST_HIP_SCANA = 1: from 10 000 rows on)
    instead of k_scan_p2.  9 999 rows take the small form for the first windows (new outliers then carry the table over the
    line), 10 000 and 10 001 the large one from the start; the lattice table holds 10 000 rows with exact ties."""
    case, exp = _case(name)
    h = _handle(env, dict(sequential=1))
    try:
        T.same_online(h, T.handle_online(h, case), exp, name)
        s = h.stats()
        assert s["scan_p_launches"] > 0 and s["scan_u_launches"] > 0 and s["seq_points"] == 0, s
    finally:
        h.close()


@pytest.mark.parametrize("mode", ["default", "prune2", "prune2-scanp3-0"])
def test_victims_in_a_table_of_twenty_thousand_rows(mode):
    """10 000 pairs x 20 dimensions, 2 048 of them hit: the size at which k_scan_p3<GENERAL> would run LISTED and the
    policy's own rules would choose pruned scans - a tainted handle launches none of it."""
    name = "victims-k4-10000x20"
    case, exp = _case(name)
    h = _handle(*MODES[mode])
    try:
        T.same_online(h, T.handle_online(h, case), exp, "%s [%s]" % (name, mode))
        _check_stats(case, mode, h.stats())
    finally:
        h.close()


@pytest.mark.parametrize("name", ["clean-19999x20", "clean-20000x20"])
def test_default_shard_threshold_in_a_group_of_two(name):
    """The library's own threshold (shard_min_row_dims = 400 000 rows x dimensions): 20 000 rows x 20 are split over the
    two ranks from the first window, 19 999 x 20 are not (the rows the call creates carry the table over the line later)."""
    case, exp = _case(name)
    hs, labels, stats = T.group_online(2, case, thresholds=None)
    try:
        for rank in range(2):
            T.same_online(hs[rank], labels[rank], exp, "%s rank %d of 2" % (name, rank))
            s = stats[rank]
            assert s["windows"] > 0, s
            _check_scan_u(case, s)
            if name == "clean-20000x20":
                assert s["sharded_windows"] == s["windows"], s
            else:
                assert s["sharded_windows"] < s["windows"], s
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize("mode", ["prune2", "default", "sequential1"])
def test_one_handle_tainted_clean_and_tainted_again(mode):
    """One handle through reset(): a tainted table, a clean one of the same width (the taint flag is cleared: its pruned
    chain and scalar operands come back - scan_u_launches says so in every mode, scan_p_launches with pruning forced), the
    tainted one again (operand columns and half-precision rows of the clean table are stale; both counters back at 0),
    then a clean table with the pdim filter and the victims that the filter decides.  sequential=1 keeps every table on
    the windows, where the library's own policy may hand a call to a sequential kernel."""
    h = _handle(*MODES[mode])
    try:
        for name in ("victims-k4-600x20", "clean-2000+1000x20", "victims-k4-600x20", "lattice-3000+1096x20",
                     "victims-set-params-200x20", "clean-2000+1000x20", "victims-filter-600x20"):
            case, exp = _case(name)
            h.reset()
            T.same_online(h, T.handle_online(h, case), exp, "%s on a reused handle [%s]" % (name, mode))
            _check_stats(case, mode, h.stats())
    finally:
        h.close()


def test_taint_by_set_params_first_call_is_clean():
    """The first call of the set_params cases runs untainted with k = 4 096 (pruned scans forced: the common case's chain
    runs); lowering k taints the handle and the second call launches no pruned scan."""
    case, exp = _case("victims-set-params-200x20")
    par0, X0 = case[4]["first"]
    h = _handle(*MODES["prune2"])
    try:
        h.set_params(*par0)
        first = h.online(X0)
        s = h.stats()
        assert s["scan_p_launches"] > 0 and s["scan_u_launches"] > 0, s
        h.set_params(*case[2])
        labels = h.online(case[3])
        s = h.stats()
        assert s["windows"] > 0 and s["scan_p_launches"] == 0 and s["scan_u_launches"] == 0, s
        T.same_online(h, (labels, first), exp, "set_params taint")
    finally:
        h.close()
