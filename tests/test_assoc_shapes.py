"""The association tracker's nearest previous pcore (cc_assoc_argmin: k_assoc_tiled<DP, UNIT>, k_assoc_tiled_blk,
k_assoc_merge) against the CPU oracle: (mc, mp) around the edges of the 64-lane tiles, the 256-row workgroups, the
32-row staging tiles and the sub-ranges of previous pcores; d across every compiled width and the blocked form; the
unit operand (k = 4, entries 1 or k), the dividing form (k = 3) and a foreign preference entry under k = 4; exact ties
on both sides of a sub-range boundary; all distances equal; distances that overflow to +inf for every candidate.
Indices and distances are compared for equality, no tolerance."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

MC = (1, 63, 64, 65, 255, 256, 257, 5000)
MP = (1, 31, 32, 33, 1023, 1025, 5000)
DIMS = (1, 3, 4, 5, 8, 13, 16, 17, 20, 21, 24, 25, 40, 41, 64, 65, 128, 129, 300)
FORMS = ("k4", "k3", "foreign")
TQ = 32  # CC_ASSOC_TQ


def sub_ranges(mc, mp):
    """(S, per) as cc_assoc_argmin and k_assoc_tiled derive them on one GPU."""
    ctiles = (mc + 255) // 256
    S = max(1, min((mp + TQ - 1) // TQ, (1024 + ctiles - 1) // ctiles))
    return S, (mp + S - 1) // S


def make_case(seed, mc, mp, d, form):
    """(k, cur, pref, prev, tied): random centroids; previous pcores just before and just after a sub-range boundary
    (and in the last sub-range) are copies of one another, and some current pcores lie on that copy or beside it."""
    rng = np.random.default_rng(seed)
    k = 3.0 if form == "k3" else 4.0
    cur = rng.random((mc, d))
    pref = np.where(rng.random((mc, d)) < 0.5, k, 1.0)
    if form == "foreign":
        pref[rng.integers(0, mc), rng.integers(0, d)] = 2.5
    prev = rng.random((mp, d))
    S, per = sub_ranges(mc, mp)
    copies = sorted({min(mp - 1, per - 1), min(mp - 1, per), mp - 1})
    for q in copies[1:]:
        prev[q] = prev[copies[0]]
    tied = rng.choice(mc, min(mc, 4), replace=False)
    cur[tied[0]] = prev[copies[0]]                                             # distance 0 to every copy
    cur[tied[1:]] = prev[copies[0]] + rng.normal(0.0, 1e-4, (len(tied) - 1, d))  # the same distance to every copy
    return k, cur, pref, prev, (tied, copies)


def check(hd, k, cur, pref, prev, what):
    from oracle import oracle as O
    hd.set_params(0.01, 0.01, k, 0.5, 1.0, 0.0, 0.1, 0.01, 0.1, cur.shape[1])
    gi, gd = hd.assoc_argmin(cur, pref, prev)
    oi, od = O.assoc_argmin(cur, pref, prev)
    bad = np.flatnonzero(gi != oi)
    assert len(bad) == 0, "%s: index of current pcore %d: %d / %d (%d differ)" % (what, bad[0], gi[bad[0]], oi[bad[0]], len(bad))
    if prev.shape[0] > 0:
        bad = np.flatnonzero(gd != od)
        assert len(bad) == 0, "%s: distance of current pcore %d: %r / %r (%d differ)" % (what, bad[0], gd[bad[0]], od[bad[0]], len(bad))
    return oi, od


@pytest.fixture(scope="module")
def hd():
    from chronoclust_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


@pytest.mark.parametrize("mc", MC)
def test_assoc_tile_and_sub_range_edges(hd, mc):
    """Every (mc, mp); d and the operand form rotate so that each mc meets several widths and all three forms."""
    for j, mp in enumerate(MP):
        i = MC.index(mc) * len(MP) + j
        d, form = DIMS[(5 * i + 2) % len(DIMS)], FORMS[i % 3]
        k, cur, pref, prev, (tied, copies) = make_case(i, mc, mp, d, form)
        oi, od = check(hd, k, cur, pref, prev, "mc=%d mp=%d d=%d %s" % (mc, mp, d, form))
        # the structure is there, on the oracle's answer: the planted ties decide, and the first copy wins
        assert oi[tied[0]] == copies[0] and od[tied[0]] == 0.0
        assert d < 3 or (oi[tied] == copies[0]).all()  # (in one or two dimensions a random point may lie closer)
        S, per = sub_ranges(mc, mp)
        if mp >= 1023:
            assert S > 1 and copies[:2] == [per - 1, per]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d", DIMS)
def test_assoc_every_width_and_form(hd, d, form):
    """257 current pcores (a second workgroup with one valid lane) x 1 025 previous ones (33 sub-ranges of 32 rows, the
    last one a single row) at every width, in all three operand forms."""
    k, cur, pref, prev, (tied, copies) = make_case(7000 + d, 257, 1025, d, form)
    assert ((pref == 1.0) | (pref == k)).all() == (form != "foreign")
    oi, od = check(hd, k, cur, pref, prev, "d=%d %s" % (d, form))
    assert oi[tied[0]] == copies[0] and len(np.unique(oi)) > 100


SUB_RANGE_SHAPES = ((5, 65), (70, 67), (5000, 1025), (2600, 3009), (5000, 1665))


@pytest.mark.parametrize("d", (3, 16, 40, 128, 300))
def test_assoc_uneven_and_empty_sub_ranges(hd, d):
    """Sub-ranges that are not whole staging tiles (mp = 65, 67: S = 3, per = 22, 23) and sub-ranges that start beyond
    the last previous pcore and report no candidate (index -1 in k_assoc_merge's input), which takes an S limited by
    the grid: mp = 1 665 under 20 workgroup rows (S = 52, per = 33, 51 * 33 = 1 683: the last one is empty) and
    mp = 3 009 under 11 (S = 94, per = 33: the last two are empty)."""
    for mc, mp in SUB_RANGE_SHAPES:
        k, cur, pref, prev, _ = make_case(d * 100 + mp, mc, mp, d, "k4" if d % 2 else "k3")
        check(hd, k, cur, pref, prev, "mc=%d mp=%d d=%d" % (mc, mp, d))


def test_sub_range_shapes_hold_what_they_are_for():
    """Integer arithmetic only: uneven sub-ranges and empty last sub-ranges occur among SUB_RANGE_SHAPES."""
    sp = [sub_ranges(mc, mp) + (mp,) for mc, mp in SUB_RANGE_SHAPES]
    assert sum(1 for S, per, mp in sp if per % TQ != 0) >= 3
    assert sum(1 for S, per, mp in sp if (S - 1) * per >= mp) >= 2 and any((S - 2) * per >= mp for S, per, mp in sp), sp


@pytest.mark.parametrize("d", (4, 24, 64, 129))
def test_assoc_all_distances_equal(hd, d):
    """Every previous pcore is the same point: whatever the sub-range, index 0 wins."""
    rng = np.random.default_rng(d)
    for mc, mp, k in ((257, 1025, 4.0), (65, 5000, 3.0)):
        cur = rng.random((mc, d))
        pref = np.where(rng.random((mc, d)) < 0.5, k, 1.0)
        prev = np.tile(rng.random((1, d)), (mp, 1))
        oi, od = check(hd, k, cur, pref, prev, "equal mc=%d mp=%d d=%d" % (mc, mp, d))
        assert (oi == 0).all() and (od > 0.0).all()


@pytest.mark.parametrize("d", (1, 8, 40, 128, 300))
def test_assoc_overflow_to_inf_for_every_candidate(hd, d):
    """Finite centroids 1e200 apart in one dimension: every squared distance is +inf, nothing is ever `<` the running
    minimum - the first previous pcore wins with distance +inf on both sides, in every sub-range form."""
    rng = np.random.default_rng(d)
    for mc, mp, k in ((65, 33, 4.0), (257, 1025, 3.0), (256, 5000, 4.0)):
        cur = rng.random((mc, d))
        cur[:, d // 2] = 1e200
        prev = rng.random((mp, d))
        prev[:, d // 2] = -1e200
        pref = np.where(rng.random((mc, d)) < 0.5, k, 1.0)
        oi, od = check(hd, k, cur, pref, prev, "inf mc=%d mp=%d d=%d" % (mc, mp, d))
        assert (oi == 0).all() and np.isposinf(od).all()


def test_assoc_no_previous_pcores(hd):
    """mp == 0: indices only (-1 on both sides; the distance is +inf here, 0.0 in the oracle, None in the reference)."""
    for mc, d in ((1, 3), (257, 16), (300, 129)):
        k, cur, pref, _, _ = make_case(mc, mc, 1, d, "k4")
        oi, _ = check(hd, k, cur, pref, np.zeros((0, d)), "mp=0 mc=%d d=%d" % (mc, d))
        assert (oi == -1).all()


@pytest.mark.parametrize("world", (2, 3))
def test_assoc_sharded_against_oracle(world):
    """Current pcores split over the ranks of an in-process group (blocks of single rows), indices and distances
    all-gathered: every rank against the oracle."""
    import threading
    from chronoclust_amd import _lib
    from oracle import oracle as O
    cases = [make_case(90 + i, mc, mp, d, form) for i, (mc, mp, d, form) in enumerate(
        ((1, 33, 5, "k4"), (257, 1025, 20, "k3"), (1000, 700, 129, "k4"), (64, 31, 64, "foreign")))]
    hs = [_lib.Handle(0) for _ in range(world)]
    _lib.comm_init_local(hs)
    out, errors = [[] for _ in range(world)], [None] * world

    def work(rank):
        try:
            hs[rank].set_shard_thresholds(0, 0)
            for k, cur, pref, prev, _ in cases:
                hs[rank].set_params(0.01, 0.01, k, 0.5, 1.0, 0.0, 0.1, 0.01, 0.1, cur.shape[1])
                out[rank].append(hs[rank].assoc_argmin(cur, pref, prev))
        except BaseException as e:  # noqa: BLE001 - reported after the join
            errors[rank] = e
            try:
                hs[rank].comm_destroy()
            except Exception:
                pass

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for h in hs:
        h.close()
    for e in errors:
        if e is not None:
            raise e
    for (k, cur, pref, prev, _), *got in zip(cases, *out):
        oi, od = O.assoc_argmin(cur, pref, prev)
        for rank, (gi, gd) in enumerate(got):
            assert np.array_equal(gi, oi) and np.array_equal(gd, od), (rank, cur.shape, prev.shape)
