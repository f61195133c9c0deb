"""CPU tests of the two pure host objects behind a batch of windows: the launch geometry of the batch (csrc/cc_batch.h through
cc_batch_plan) and the hand-over rule between the windows and the sequential kernel (cc::SeqHandover of csrc/cc_policy.h
through cc_seq_handover_replay).  No GPU, no clock.  Every expected value is worked out by hand from the rule as the code
states it - the arithmetic stands beside it -, none is what the code returned.  tests/test_host_sanitizers.py runs the
same cases (every test_* function of this module) against the sanitizer builds."""
import pytest

from chronoclust_amd import _lib
from chronoclust_amd._lib import LONG_LIST_SMALL, LONG_LIST_SPLIT, LONG_NONE, LONG_ROWS_SMALL, LONG_ROWS_SPLIT

# a settled full-size batch on a 256-CU device: everything allowed, nothing seen yet
BASE = dict(window=49152, win_cfg=4096, S_cfg=16, n_cus=256, prune_now=0, prune_wgs_per_cu=2, plain_wgs_per_cu=3,
            decide_threads=256, chain_threads=64, commit_threads=256, allow_claims=1, allow_long=1, allow_heavy=1, allow_prep=1,
            m_rows=5000, n_heavy=0, long_seen=0, long_few=1, long_avg=1, batch_windows=16, points_left=10 ** 6)


def plan(**over):
    return _lib.batch_plan(**dict(BASE, **over))


def test_windows_now_stops_at_the_end_of_the_range():
    assert plan(points_left=10000)["windows_now"] == 3   # ceil(10 000 / 4 096) = 3 < 16
    assert plan(points_left=0)["windows_now"] == 1       # never less than one
    assert plan(points_left=10 ** 6)["windows_now"] == 16  # ceil(10^6 / 4 096) = 245: the batch's 16
    assert plan(points_left=4096 * 3)["windows_now"] == 3 and plan(points_left=4096 * 3 + 1)["windows_now"] == 4


def test_grid_width_is_the_batch_window_at_least_64():
    assert plan(win_cfg=32)["gw"] == 64 and plan(win_cfg=4096)["gw"] == 4096
    assert plan(window=8192, win_cfg=49152)["gw"] == 8192  # never beyond the configured window


def test_sparse_cap_is_a_sixteenth_of_the_window_in_whole_tiles():
    # min(49 152 / 16, max(64, ceil(gw / 16 / 64) * 64))
    assert plan(win_cfg=64)["sparse_cap"] == 64       # 64 / 16 = 4 -> one tile
    assert plan(win_cfg=4096)["sparse_cap"] == 256    # 4 096 / 16 = 256 = 4 tiles
    assert plan(win_cfg=49152)["sparse_cap"] == 3072  # 49 152 / 16 = 3 072 = 48 tiles, the most
    assert plan(win_cfg=1040)["sparse_cap"] == 128    # 1 040 / 16 = 65 -> 2 tiles


@pytest.mark.parametrize("threads, b64, b4096, rb49152", [
    # one 32-lane group per point: threads / 32 points per workgroup -> gw / (threads / 32) workgroups;
    # k_commit_b at most 1 024 * (256 / threads): 49 152 points would be 24 576 / 12 288 / 6 144
    (64, 32, 2048, 4096), (128, 16, 1024, 2048), (256, 8, 512, 1024)])
def test_blocks_at_the_three_legal_thread_counts(threads, b64, b4096, rb49152):
    for gw, want in ((64, b64), (4096, b4096)):
        p = plan(win_cfg=gw, decide_threads=threads, chain_threads=threads, commit_threads=threads)
        assert (p["dblocks"], p["cblocks"], p["rblocks"]) == (want, want, want), (gw, p)
    p = plan(win_cfg=49152, decide_threads=threads, chain_threads=threads, commit_threads=threads)
    assert p["dblocks"] == p["cblocks"] == 49152 * 32 // threads and p["rblocks"] == rb49152
    # 65 points at 256 threads: 8 per workgroup -> 9; each kernel by its own knob
    p = plan(win_cfg=65, decide_threads=256, chain_threads=64, commit_threads=128)
    assert (p["dblocks"], p["cblocks"], p["rblocks"]) == (9, 33, 17)
    with pytest.raises(ValueError):
        plan(decide_threads=96)


def test_scan_rows_up_to_1024_table_rows():
    assert [plan(m_rows=m)["scan_rows"] for m in (0, 1, 1024, 1025)] == [0, 1, 1024, 0]
    assert [plan(m_rows=m, allow_claims=0)["scan_rows"] for m in (1, 1024)] == [0, 0]
    # the long chains of those rows: with k_claims only
    assert plan(m_rows=200)["long_rows"] == 200 and plan(m_rows=200, allow_long=0)["long_rows"] == 0
    assert plan(m_rows=200, allow_claims=0)["long_rows"] == 0


def test_chain_long_form_by_rows():
    # rows <= 64: prepared (PREP ahead of k_chain) and SPLIT; <= 256: SPLIT; beyond: the small workgroups
    want = {64: (1, LONG_ROWS_SPLIT, LONG_ROWS_SPLIT), 65: (0, LONG_NONE, LONG_ROWS_SPLIT), 256: (0, LONG_NONE, LONG_ROWS_SPLIT),
            257: (0, LONG_NONE, LONG_ROWS_SMALL), 1024: (0, LONG_NONE, LONG_ROWS_SMALL)}
    for rows, w in want.items():
        p = plan(m_rows=rows, long_seen=1)  # (long_seen plays no part while k_claims serves the table)
        assert (p["prep"], p["prep_form"], p["long_form"]) == w and p["long_rows"] == rows and p["long_listed"] == 0, rows
    p = plan(m_rows=64, allow_prep=0)
    assert (p["prep"], p["prep_form"], p["long_form"]) == (0, LONG_NONE, LONG_ROWS_SPLIT)
    p = plan(m_rows=64, allow_long=0)
    assert (p["prep"], p["prep_form"], p["long_form"], p["long_rows"]) == (0, LONG_NONE, LONG_NONE, 0)


def test_chain_long_form_by_list():
    # scan_rows == 0 (5 000 rows): over the list k_decide keeps, once a batch has seen long chains; few: prepared + SPLIT
    for seen, few, w in ((0, 0, (0, 0, LONG_NONE, LONG_NONE)), (0, 1, (0, 0, LONG_NONE, LONG_NONE)),
                         (1, 1, (1, 1, LONG_LIST_SPLIT, LONG_LIST_SPLIT)), (1, 0, (1, 0, LONG_NONE, LONG_LIST_SMALL))):
        p = plan(long_seen=seen, long_few=few)
        assert (p["long_listed"], p["prep"], p["prep_form"], p["long_form"]) == w, (seen, few)
    p = plan(long_seen=1, long_few=1, allow_prep=0)
    assert (p["long_listed"], p["prep"], p["prep_form"], p["long_form"]) == (1, 0, LONG_NONE, LONG_LIST_SPLIT)
    p = plan(long_seen=1, long_few=1, allow_long=0)
    assert (p["long_listed"], p["prep"], p["prep_form"], p["long_form"]) == (0, 0, LONG_NONE, LONG_NONE)
    # claims off on a small table: no k_claims, so its chains are listed like a large table's
    p = plan(m_rows=50, allow_claims=0, long_seen=1, long_few=1)
    assert (p["long_rows"], p["long_listed"], p["long_form"]) == (0, 1, LONG_LIST_SPLIT)


def test_long_cap_follows_the_previous_batch_while_chains_are_few():
    assert plan(long_few=1, long_avg=1)["long_cap"] == 10     # 2 * 1 + 8
    assert plan(long_few=1, long_avg=64)["long_cap"] == 136   # 2 * 64 + 8
    assert plan(long_few=0, long_avg=65)["long_cap"] == 512   # not few: CC_LONG_CAP
    assert plan(long_few=1, long_avg=400)["long_cap"] == 512  # never beyond it


def test_heavy_rows_are_gathered_on_large_tables_only():
    assert plan(n_heavy=3)["heavy_on"] == 1 and plan(n_heavy=0)["heavy_on"] == 0
    assert plan(n_heavy=3, allow_heavy=0)["heavy_on"] == 0
    assert plan(n_heavy=3, m_rows=1024)["heavy_on"] == 0       # k_claims serves the table
    assert plan(n_heavy=3, m_rows=1024, allow_claims=0)["heavy_on"] == 1


def test_partials_per_point():
    # pruned: as few sub-ranges as fill the machine once - 256 CUs x 2 workgroups = 512 over the batch's point tiles
    assert plan(prune_now=1, win_cfg=4096)["S"] == 8     # 512 / 64 tiles = 8 <= S_cfg
    assert plan(prune_now=1, win_cfg=1024)["S"] == 16    # 512 / 16 tiles = 32 -> S_cfg
    assert plan(prune_now=1, win_cfg=49152)["S"] == 1    # 512 / 768 tiles = 0 -> at least one
    # plain: scan_partials_for(64, 16, 768).  64 tiles x 16 = 1 024 workgroups on 768 resident run two rounds, the second a
    # third full (efficiency 2/3); 64 x 12 = 768 fill one round exactly (efficiency 1): 12, the first s from 16 down that
    # reaches it (15, 14, 13: 960, 896, 832 workgroups still take two rounds)
    assert plan(win_cfg=4096, S_cfg=16, n_cus=256, plain_wgs_per_cu=3)["S"] == 12
    # S_cfg = 8: 64 s <= 512 workgroups never fill the 768, the efficiency is 64 s / 768 itself and the largest s wins
    assert plan(win_cfg=4096, S_cfg=8, n_cus=256, plain_wgs_per_cu=3)["S"] == 8


# ---- cc::SeqHandover ----

def batch(bad, rate, possible=1, more=1, seq_r=0, guess=700.0):
    return dict(chunk_event=0, bad=bad, rate=rate, possible=possible, more=more, seq_r_applies=seq_r, rate_guess=guess)


def chunk(got, rate, size=8192, use_g=0, allow_seq_g=1, possible=1, more=1, wide=0):
    return dict(chunk_event=1, got=got, rate=rate, chunk=size, use_g=use_g, allow_seq_g=allow_seq_g, possible=possible, more=more,
                wide=wide)


CONTINUE, PROBE, WINDOWS = 0, 1, 2
# d = 20, guess 700 points / ms; truncating windows at 100 points / ms: on after the SECOND bad batch
TAKEOVER = [batch(1, 100.0), batch(1, 100.0)]
STINT = [chunk(8192, 500.0)] * 4  # 4 x 8 192 = the first stint's 32 768 points, at 500 points / ms


def replay(events, mode=0, possible=1, sticky=0):
    return _lib.seq_handover_replay(mode, possible, sticky, events)


def test_takeover_after_two_bad_batches_slower_than_the_guess():
    out, stint = replay(TAKEOVER + [batch(1, 100.0)])
    assert out == [0, 0, 1, 1] and stint == [32768] * 4
    assert replay([batch(1, 100.0, seq_r=1)])[0] == [0, 1]  # the register kernel: one bad batch is enough
    assert replay([batch(1, 100.0), batch(0, 100.0), batch(1, 100.0)])[0] == [0, 0, 0, 0]  # not in a row
    assert replay([batch(1, 800.0)] * 5)[0] == [0] * 6      # windows at 800 points / ms beat the guess: never
    assert replay([batch(1, 100.0, more=0)] * 3)[0] == [0] * 4  # nothing left to hand over
    # a batch that committed nothing has no rate: the last one stands (800, then 100)
    assert replay([batch(1, 800.0), batch(1, 0.0)])[0] == [0, 0, 0]
    assert replay([batch(1, 100.0), batch(1, 0.0)])[0] == [0, 0, 1]


def test_a_stint_ends_as_a_probe_and_doubles_while_the_windows_stay_slower():
    out, stint = replay(TAKEOVER + STINT)
    assert out[3:] == [CONTINUE, CONTINUE, CONTINUE, PROBE]  # 32 768 - 4 x 8 192 = 0 left
    # the probe batch is bad and slower (100 < 500): back for twice as long
    ev = TAKEOVER + STINT + [batch(1, 100.0)]
    out, stint = replay(ev)
    assert out[-1] == 1 and stint[-1] == 65536
    # ... and again, each stint as many chunks as it is long: 128 k, 256 k, 512 k, 1 M, and 1 M it stays
    for want in (131072, 262144, 524288, 1048576, 1048576):
        n = stint[-1] // 8192
        ev = ev + [chunk(8192, 500.0)] * n + [batch(1, 100.0)]
        out, stint = replay(ev)
        assert out[-n - 1:-1] == [CONTINUE] * (n - 1) + [PROBE] and out[-1] == 1 and stint[-1] == want, want
    # a probe batch that is not bad, or not slower, resets the length and stays on the windows
    base = TAKEOVER + STINT + [batch(1, 100.0)] + [chunk(8192, 500.0)] * 8  # (in the 65 536 stint's probe)
    assert replay(base)[0][-1] == PROBE and replay(base)[1][-1] == 65536
    for probe_batch in (batch(0, 100.0), batch(1, 600.0)):
        out, stint = replay(base + [probe_batch])
        assert out[-1] == 0 and stint[-1] == 32768
    # ... and the takeover then needs two bad batches in a row again, of which a bad probe batch is the first
    assert replay(base + [batch(0, 100.0), batch(1, 100.0)])[0][-1] == 0
    assert replay(base + [batch(0, 100.0), batch(1, 100.0), batch(1, 100.0)])[0][-1] == 1
    assert replay(base + [batch(1, 600.0), batch(1, 100.0)])[0][-1] == 1


def test_a_short_chunk_does_not_update_the_measured_rate():
    # the stint's last 500 points come in a chunk of their own, at a rate of 10 (32 768 = 3 x 8 192 + 7 692 + 500)
    ev = TAKEOVER + [chunk(8192, 500.0)] * 3 + [chunk(8192 - 500, 500.0), chunk(500, 10.0)]
    out, _ = replay(ev)
    assert out[3:] == [CONTINUE] * 4 + [PROBE]
    # had 10 points / ms become the measured rate, windows at 100 would no longer be slower: they are (500 stands)
    assert replay(ev + [batch(1, 100.0)])[0][-1] == 1
    # a chunk of 1 024 points does count: 100 is not below 10, the windows keep the stream
    ev = TAKEOVER + [chunk(8192, 500.0)] * 3 + [chunk(8192 - 1024, 500.0), chunk(1024, 10.0)]
    assert replay(ev + [batch(1, 100.0)])[0][-2:] == [PROBE, 0]


def test_modes_and_possible():
    bad = [batch(1, 1.0)] * 4
    assert replay(bad, mode=1, sticky=1)[0] == [0] * 5              # mode 1: never
    assert replay([batch(1, 1.0, possible=0)] * 4, possible=0, sticky=1)[0] == [0] * 5  # a group, no_create: never
    assert replay([batch(1, 1.0, possible=0)] * 4, mode=2, possible=0)[0] == [0] * 5
    assert replay([], mode=0, sticky=1)[0] == [1] and replay([], mode=0, sticky=0)[0] == [0]  # the previous call ended on it
    # mode 2: on whenever possible, and a stint never ends by its length (100 chunks = 819 200 points > 32 768)
    out, _ = replay([chunk(8192, 500.0)] * 100 + [batch(0, 5000.0)], mode=2)
    assert out == [1] + [CONTINUE] * 100 + [1]
    # ... only when the table leaves no room: back to the windows for good, and on again after their batch
    out, _ = replay([chunk(100, 500.0, use_g=1), batch(0, 5000.0)], mode=2)
    assert out == [1, WINDOWS, 1]
    with pytest.raises(ValueError):
        replay([], mode=3)


def test_a_short_chunk_goes_back_to_the_windows_for_good():
    # k_seq's image is full with points left and k_seq_g is not allowed: for good, not as a probe - also at the stint's end
    assert replay(TAKEOVER + [chunk(3000, 500.0, allow_seq_g=0)])[0][-1] == WINDOWS
    assert replay(TAKEOVER + [chunk(8192, 500.0)] * 3 + [chunk(8192, 500.0, size=16384, allow_seq_g=0)])[0][-1] == WINDOWS
    # with k_seq_g allowed the stint goes on (k_seq_g takes the next chunk); k_seq_g's own short chunk ends it
    assert replay(TAKEOVER + [chunk(3000, 500.0)])[0][-1] == CONTINUE
    assert replay(TAKEOVER + [chunk(3000, 500.0, use_g=1)])[0][-1] == WINDOWS
    # the sequential kernel is no longer possible (the table outgrew the image, k_seq_g off): for good
    assert replay(TAKEOVER + [chunk(8192, 500.0, possible=0)])[0][-1] == WINDOWS
    # the call's last chunk, or no windows to go back to (wide): nothing to hand back
    assert replay(TAKEOVER + [chunk(3000, 500.0, allow_seq_g=0, more=0)])[0][-1] == CONTINUE
    assert replay([chunk(3000, 500.0, use_g=1, wide=1)], mode=2)[0][-1] == CONTINUE
    # after "for good" the next batch is no probe: one bad batch does not bring the kernel back, two do
    ev = TAKEOVER + [chunk(3000, 500.0, allow_seq_g=0)]
    assert replay(ev + [batch(1, 100.0)])[0][-1] == 0 and replay(ev + [batch(1, 100.0)] * 2)[0][-1] == 1
