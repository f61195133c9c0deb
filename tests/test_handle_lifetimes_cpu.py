"""What the itineraries of tests/lifetime_util.py contain, without a GPU: every predecessor -> successor pair the lives exist
for occurs (padded / ladder / same padded width are cc::scan_width's own statement), every band of widths is entered from a
wider and from a narrower predecessor, every new table case holds joins to pcores, joins to outliers and creations in the
oracle's result, the emptied table is empty in the oracle, and no step is conditional on the mode."""
import numpy as np

import lifetime_util as L
import table_util as T


def _names(life, mode="sequential1"):
    return [s["case"] for s in L.LIVES[life][mode]]


def test_every_mode_has_an_explicit_itinerary_of_the_same_tables():
    assert set(L.MODES) == set(L.MODE_NAMES) == {"prune2", "default", "sequential1"}
    for life, by_mode in L.LIVES.items():
        assert set(by_mode) == set(L.MODE_NAMES), life
        tables = [_names(life, m) for m in L.MODE_NAMES]
        assert tables[0] == tables[1] == tables[2], life       # (the modes differ in tuning, never in the steps taken)
        for steps in by_mode.values():
            assert len(steps) >= 4 and all(set(s) == {"case", "tuning", "stats"} for s in steps)
    for order, keys in L.ORDERS.items():
        assert sorted(keys) == sorted(L.STREAMS) and len(keys) >= 12
    assert L.ORDERS["reversed"] == L.ORDERS["forwards"][::-1]


def test_new_cases_stay_out_of_the_reference_surface_and_within_the_size_cap():
    assert not set(L.LIFE_TABLES) & set(T.ONLINE_TABLES)
    used = {s["case"] for by_mode in L.LIVES.values() for steps in by_mode.values() for s in steps}
    used |= set(L.READONLY) | {L.EMPTIED_FIRST, L.EMPTIED_THEN}
    assert set(L.LIFE_TABLES) <= used
    for name in used:
        c = L.case(name)[0]
        rows, n = L.rows_of(c), len(c[3])
        assert rows <= 10001 and n <= 2048, (name, rows, n)
        if name in L.LIFE_TABLES:
            assert rows * n <= L.MAX_ROWS_POINTS, (name, rows, n)


def test_new_cases_hold_joins_to_both_lists_and_creations():
    for name in L.LIFE_TABLES:
        c, exp, off = L.case(name)
        assert not c[4]["tainted"], name
        path = exp["path"]
        assert (path == 0).any() and ((path == 1) | (path == 5)).any() and (path == 2).any(), (name, np.unique(path))
        assert off[0]["num_core"] > 0, name


def test_widths_life_shrinks_what_the_predecessor_left_large():
    names = _names("widths")
    d = [L.params(n)[0] for n in names]
    dp = [L.scan_rule(n)[0] for n in names]
    assert d == [64, 13, 14, 63, 13, 20]
    assert dp == [64, 14, 14, 64, 14, 20]                      # cc::scan_width: 13 -> 14 and 63 -> 64 are padded
    kinds = ["ladder" if a == b else "padded" for a, b in zip(d, dp)]
    pairs = list(zip(zip(kinds, dp), zip(kinds[1:], dp[1:])))
    assert (("ladder", 64), ("padded", 14)) in pairs           # a ladder width, then a mirror is built for the first time
    assert (("padded", 14), ("ladder", 14)) in pairs           # a ladder width of the DP of the mirror just used
    assert (("ladder", 14), ("padded", 64)) in pairs
    assert (("padded", 64), ("padded", 14)) in pairs           # pad_stride kept from DP 64 while DP is 14
    assert (("padded", 14), ("ladder", 20)) in pairs
    mirrors = [n for n, k_, p in zip(names, kinds, dp) if k_ == "padded" and p == 14]
    assert len(set(mirrors)) == 2                              # a mirror of the same DP with other contents
    rows = [L.rows_of(L.case(n)[0]) for n in names]
    assert all(a > b for a, b in zip(rows, rows[1:])), rows    # rows of the old table lie beyond the new m_rows
    for n in names:
        assert L.scan_rule(n)[1] and L.scan_rule(n)[2] != "none", n


def test_regimes_life_visits_every_kernel_family_in_order():
    for mode in L.MODE_NAMES:
        names = _names("regimes", mode)
        d = [L.params(n)[0] for n in names]
        rows = [L.rows_of(L.case(n)[0]) for n in names]
        assert d == [40, 3, 80, 200, 8, 20, 20] and [L.band(x) for x in d] == ["ladder", "registers", "hbm", "wide", "staged",
                                                                              "ladder", "ladder"]
        assert rows[0] == 1500 and rows[1] == 34 and rows[5] == 10001 and rows[6] == 30
        steps = L.LIVES["regimes"][mode]
        assert max(L.tuning_at(mode, steps, i).get("window", 1 << 30) for i in range(len(steps))) <= 4096
        assert max(d) <= 300
    dflt = L.LIVES["regimes"]["default"]
    assert L.tuning_at("default", dflt, 1)["sequential"] == 2 and dflt[1]["stats"] == "sequential2"   # k_seq_r is asked for ...
    assert L.tuning_at("default", dflt, 2)["sequential"] == 0                                          # ... and the policy gets its say back
    for mode in ("prune2", "sequential1"):
        assert all(L.tuning_at(mode, L.LIVES["regimes"][mode], i)["sequential"] == 1 for i in range(7))


def test_k_filter_and_taint_lives_change_one_thing_at_one_width():
    ks = [L.params(n) for n in _names("k")]
    assert [p[3] for p in ks] == [4.0, 3.0, 0.5, 4.0] and {p[0] for p in ks} == {20}
    assert [p[2] for p in ks] == [True, False, True, True] and not any(p[4] for p in ks)
    assert [L.scan_rule(n)[2] for n in _names("k")] == ["common", "general", "common", "common"]
    fs = [L.params(n) for n in _names("filter")]
    assert [p[1] for p in fs] == [True, False, True, False, True] and {p[0] for p in fs} == {14}
    for mode in L.MODE_NAMES:      # only lookahead scans read the scan copies; several windows per table
        steps = L.LIVES["filter"][mode]
        assert all(L.tuning_at(mode, steps, i)["lookahead"] == 3 and L.tuning_at(mode, steps, i)["window"] == 64
                   for i in range(len(steps)))
    assert all(len(L.case(n)[0][3]) > 4 * 64 for n in _names("filter"))
    ts = [L.params(n) for n in _names("taint")]
    assert [p[4] for p in ts] == [False, True, False, True, False] and {p[0] for p in ts} == {32}


def test_tuning_life_moves_every_knob_between_consecutive_steps():
    for mode in L.MODE_NAMES:
        steps = L.LIVES["tuning"][mode]
        tun = [L.tuning_at(mode, steps, i) for i in range(len(steps))]
        for key, want in (("window", [(4096, 64), (64, 1), (1, 1024)]), ("lookahead", [(3, 2), (2, 0)]),
                          ("windows_per_sync", [(4, 1)])):
            got = [(a[key], b[key]) for a, b in zip(tun, tun[1:])]
            for pair in want:
                assert pair in got, (mode, key, pair, got)
        assert len({L.params(s["case"])[0] for s in steps}) == 1


def _entered(widths_in_order):
    """width -> (has a narrower predecessor, has a wider one) over sequences of widths."""
    out = {}
    for seq in widths_in_order:
        for a, b in zip(seq, seq[1:]):
            lo, hi = out.get(b, (False, False))
            out[b] = (lo or a < b, hi or a > b)
    return out


def test_every_band_of_tables_is_entered_from_both_sides():
    seqs = [[L.params(n)[0] for n in _names(life)] for life in L.LIVES]
    by_band = {}
    for d, (lo, hi) in _entered(seqs).items():
        a, b = by_band.get(L.band(d), (False, False))
        by_band[L.band(d)] = (a or lo, b or hi)
    assert set(by_band) == {"registers", "staged", "padded", "ladder", "hbm", "wide"}
    for band, (lo, hi) in by_band.items():         # (within the end bands too: d 200 behind d 256, d 3 behind d 2)
        assert lo and hi, (band, lo, hi)


def test_every_stream_width_is_entered_from_both_sides():
    dims = {key: L.stream_dim(key) for key in L.STREAMS}
    assert {1, 2, 4, 9, 17, 33, 64, 129} <= set(dims.values())
    assert max(len(X) for key in L.STREAMS for X in L.stream(key)[2]) <= 30000
    assert L.stream(("wide", 129))[2][0].shape == (1500, 129) and min(sum(len(X) for X in L.stream(key)[2]) for key in L.STREAMS) >= 300
    entered = _entered([[dims[k] for k in keys] for keys in L.ORDERS.values()])
    for d in set(dims.values()):
        lo, hi = entered[d]
        assert lo or d == min(dims.values()), d
        assert hi or d == max(dims.values()), d
    ks = {L.stream(key)[0]["k"] for key in L.STREAMS}
    assert {0.5, 1.0, 3.0, 4.0} <= ks
    assert any(0 < L.stream(k)[0]["pi"] < dims[k] for k in L.STREAMS) and any(L.stream(k)[0]["pi"] in (0, dims[k]) for k in L.STREAMS)
    for order, keys in L.ORDERS.items():           # the restored state goes into a handle that last ran another width
        assert dims[keys[-1]] != dims[L.RESTORED] and L.RESTORED in keys[:-1]
    snaps = L.stream_oracle(L.RESTORED)
    assert len(snaps) == len(L.stream(L.RESTORED)[2]) + 1 and len(snaps[-2].table(0)["id"]) + len(snaps[-2].table(1)["id"]) > 0


def test_the_emptied_table_is_empty_in_the_oracle_and_ids_continue():
    e = L.emptied()
    rows = [s.rows() for s in e["decays"]]
    assert rows[-1] == 0 and rows[0] > 0 and len(rows) > 1, rows      # (one call never deletes everything: see emptied())
    assert all(a > b for a, b in zip(rows, rows[1:])), rows
    assert e["first_case"][3].shape[1] == 20 and e["then_case"][3].shape[1] == 13
    assert len(e["first"]["offline"][1]) > 0                       # clusters of the first life stay behind in the handle
    then = e["then"]
    assert then["o"].counters[0] > e["first"]["counters"][0] and then["o"].counters[1] > e["first"]["counters"][1]
    new = then["uid"][then["path"] == 2]
    assert len(new) and new.min() >= e["first"]["counters"][1] and (then["path"] == 0).any()
    pc = e["then_point_clusters"]
    assert (pc >= 0).any() and (pc < 0).any() and len(e["then_offline"][1]) > 1


def test_the_collapse_crosses_ten_thousand_rows_twice():
    c = L.collapse()
    rows = c["rows"]
    assert max(len(X) for X in c["Xs"]) <= 30000 and c["Xs"][0].shape[1] == 20 and len(c["Xs"][1]) == 500
    assert rows[0] > 10000 > rows[2] and rows[1] < rows[0] // 4 and rows[3] > 10000, rows
    for call in c["calls"]:
        assert (call["path"] == 2).any() and (call["path"] == 0).any()


def test_the_read_only_life_has_both_widths_and_sizes():
    shapes = {L.readonly(n)["X"].shape for n in L.READONLY}
    assert shapes == {(300, 13), (2048, 20)}
    for n in L.READONLY:
        r = L.readonly(n)
        assert (r["point_clusters"] >= 0).any() and (r["point_clusters"] < 0).any() and len(r["offline"][1]) > 1
        assert set(np.unique(r["exp"]["path"])) >= {0, 2}
