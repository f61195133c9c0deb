"""cc_assign without a GPU: the entry point is declared and bound, cc_stats carries its two counters at the end, and the
cases of tests/test_assign_tables.py hold what they are for - judged on the CPU oracle alone (tests/assign_util.py: one
fresh oracle per point)."""
import os
import re

import numpy as np
import pytest

import assign_util as A
from chronoclust_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cc_assign_is_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "chronoclust_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+cc_assign\s*\(([^)]*)\)\s*;", text)
    assert m, "include/chronoclust_hip.h does not declare cc_assign"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 7 and args[0].startswith("cc_handle*") and args[-1].startswith("double*"), args
    assert "cc_assign" in _lib.SYMBOLS
    res, argtypes = _lib.SYMBOLS["cc_assign"]
    assert len(argtypes) == 7
    assert callable(getattr(_lib.Handle, "assign", None))


def test_cc_stats_ends_with_the_assign_counters():
    names = [k for k, _ in _lib.CcStats._fields_]
    assert names[-2:] == ["assign_points", "assign_launches"], names[-4:]
    assert names.index("pad_rows_launches") == len(names) - 3  # appended: nothing before them moved


def test_hddstream_has_the_python_face():
    from chronoclust_amd.clustering.hddstream import HDDStream
    import chronoclust.clustering.hddstream as alias
    for name in ("assign", "assign_clusters"):
        assert callable(getattr(HDDStream, name, None)), name
        assert getattr(alias.HDDStream, name) is getattr(HDDStream, name)


FULL = ["stale-31+33x5", "stale-127+128x14", "lattice-33+33x3", "lattice-128+127x8", "lattice-129+64x13"]


@pytest.mark.parametrize("name", FULL)
def test_cases_hold_every_path_and_differ_from_the_sequential_answer(name):
    """All of paths 0, 1, 2 and 5 occur in the frozen answers, and the frozen answers are not the sequential ones: an
    implementation that runs the online phase over the points cannot pass."""
    rows, points = A.rows_points(name)
    assert rows * points <= 300000
    uid, path, dist = A.frozen(name)
    seen = set(int(p) for p in np.unique(path))
    assert {0, 1, 2, 5} <= seen, "%s: paths %r" % (name, sorted(seen))
    assert ((path == 2) == (uid == -1)).all() and ((path == 2) == (dist == -1.0)).all()
    assert (dist[path != 2] >= 0.0).all()
    s_uid, s_path = A.sequential(name)
    differ = int(((np.where(s_path == 2, -1, s_uid) != uid) | (s_path != path)).sum())
    print("%s: %d rows, %d points, paths %s, %d differ from the sequential answer" % (
        name, rows, points, dict(zip(*[x.tolist() for x in np.unique(path, return_counts=True)])), differ))
    assert differ >= 1


def test_victims_report_the_near_row_when_frozen():
    """On the tainted `victims` tables every point's frozen answer is its pair's row R (stored entries far above k), not the
    neighbour R2 that a bound with min(1, 1 / k) would prefer."""
    for name in ("victims-k4-64x13", "victims-k3-200x14"):
        pcores, outliers, par, X, meta, idx = A.case(name)
        uid, path, _ = A.frozen(name)
        t = meta["rows"]
        assert np.array_equal(uid, t.uid[meta["R"][meta["pair"][idx]]]) and (path == 0).all(), name
