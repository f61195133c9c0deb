"""The designed arrivals of tests/test_arrival_orders.py against the CPU oracle alone (no GPU): every case of
arrival_util.ARRIVAL_CASES is built, the oracle runs the online phase on it, and `check_online` asserts that the case holds its
design - per period each row's count is its L_i, every designed point was absorbed by its site's row, the first rejected member
of each breathing row, the promoting member of each outlier row and the points that change their row there are the designed
ones, each creating site has one creation.  The batch K(d) the lengths are built around is held against the line of
cc_validate.h that computes it."""
import os
import re

import numpy as np
import pytest

import arrival_util as A
import table_util as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(A.ARRIVAL_CASES))
def test_arrival_case_structure(name):
    case = A.build_arrivals(name)
    T.check_online(case, T.oracle_online(case))


def test_batch_size_is_the_kernels():
    """K = min(256, (CC_LONG_XY_DOUBLES / (2 d)) & ~7) with 6 144 staged doubles, and the limits the lengths sit on."""
    with open(os.path.join(ROOT, "chronoclust_amd", "csrc", "cc_validate.h")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "chronoclust_amd", "csrc", "cc_common.h")) as f:
        common = f.read()
    doubles = int(re.search(r"^#define CC_LONG_XY_DOUBLES (\d+)", src, re.M).group(1))
    m = re.search(r"const int K = min\((\d+), \(CC_LONG_XY_DOUBLES / \((\d+) \* d\)\) & ~(\d+)\);", src)
    assert m, "k_chain_long computes its batch otherwise"
    cap, per_dim, mask = (int(x) for x in m.groups())
    for d, want in ((3, 256), (6, 256), (12, 256), (14, 216), (20, 152), (40, 72), (64, 48)):
        assert min(cap, (doubles // (per_dim * d)) & ~mask) == A.chain_batch(d) == want, d
    assert int(re.search(r"^#define CC_LONG_QUEUE (\d+)", src, re.M).group(1)) == 2048
    assert int(re.search(r"^#define CC_CHAIN_MEMB (\d+)", common, re.M).group(1)) == 32
    assert int(re.search(r"^#define CC_LONG_CAP (\d+)", common, re.M).group(1)) == 512
    assert int(re.search(r"^#define CC_HEAVY_CAP (\d+)", common, re.M).group(1)) == 64


def test_every_designed_length_and_step_occurs():
    """Over all cases: every length of the issue's list per K, every rejection / promotion step, every d and both table sizes."""
    lengths, steps = {}, {}
    for name, kw in A.ARRIVAL_CASES.items():
        K = A.chain_batch(kw["d"])
        for sp in kw["specs"]:
            lengths.setdefault(K, set()).add(sp["L"])
            if sp["kind"] in ("breath", "promo"):
                steps.setdefault((sp["kind"], K), set()).add(sp["s"])
    for K in (256, 216, 152, 72, 48):
        assert {1, 31, 32, 33, 34, K - 1, K, K + 1, 2 * K, 2 * K + 1, 2047} <= lengths[K], (K, sorted(lengths[K]))
        assert {1, 32, 33, K - 1, K, K + 1} <= steps[("breath", K)], K
    assert {2048, 2049, 8191, 8192, 8193, 49152} <= set().union(*lengths.values())
    for K in (256, 152, 72):
        assert {1, 32, 33, K - 1, K, K + 1} <= steps[("promo", K)], K
    assert {kw["d"] for kw in A.ARRIVAL_CASES.values()} == {3, 6, 14, 20, 40, 64}
    assert any(sp["kind"] == "create" and sp["L"] in (34, 258) for kw in A.ARRIVAL_CASES.values() for sp in kw["specs"])


def test_robin_members_are_evenly_apart_and_bursts_where_designed():
    """The schedule itself: a robin row alone at its phase has members exactly W / L apart; the bursts straddle what they name."""
    owner = A._schedule(4096, [A.plain(256, ("robin", 3)), A.plain(0, ("fill",))])
    assert np.array_equal(np.flatnonzero(owner == 0), 3 + 16 * np.arange(256))
    case = A.build_arrivals("bursts-robin-d6")
    lab, specs = case[4]["lab"][:4096], case[4]["specs"]
    runs = {i: np.flatnonzero(lab == i) for i, sp in enumerate(specs) if sp["pat"][0] == "burst"}
    for i, at in runs.items():
        assert np.array_equal(at, at[0] + np.arange(len(at))), "row %d is no burst" % i
    firsts, lasts = {int(at[0]) for at in runs.values()}, {int(at[-1]) for at in runs.values()}
    assert 0 in firsts and 4095 in lasts
    assert any(at[0] // 64 != at[-1] // 64 and len(at) < 64 for at in runs.values())
    assert any(at[0] // 16 != at[-1] // 16 for at in runs.values())
    case = A.build_arrivals("headtail-robin-d6")
    lab = case[4]["lab"][:4096]
    for i in (0, 1):
        at = np.flatnonzero(lab == i)
        assert (at[:32] < 64).all() and (at[-20:] >= 4096 - 64).all() and at[32] >= 2048
