"""The referee of the read-only assignment (cc_assign) and the cases its tests share.

For a case (pcores, outliers, par, X, meta) of tests/table_util.py the expected answer for point i is the reference's loop
for that one point on a table of its own: a fresh make_oracle(par, pcores, outliers), one call of
online_microcluster_maintenance(X[i:i+1], 0, reset_param=False, offline=False), labels_uid[0] and paths[0] - with the uid
replaced by -1 where the path is 2 (the frozen call consumes no creation number).  The expected distance is
oracle.projected_distance(cen, pref, x) of the reported row, -1.0 for path 2.  About 10 us per injected row and point:
cases are kept below 300 000 rows x points by taking subsets of their points; every answer is computed once per session."""
import numpy as np

import table_util as T

# name -> (how the case is built, which of its points are assigned).  The names of table_util.ONLINE_TABLES keep theirs.
EXTRA = {
    "stale-filter-33+31x129": lambda: T.stale(seed=902, m_p=33, m_o=31, d=129, n=70, filt=True),
    "stale-20+10x1024": lambda: T.stale(seed=901, m_p=20, m_o=10, d=1024, n=40),
}
SUBSET = {
    "stale-k0.5-600x32": slice(None, None, 4),
    "victims-outliers-k3-500x40": slice(0, 64),
    "lattice-1000+500x14": slice(None, None, 16),
}

_cases, _frozen = {}, {}


def case(name):
    """(pcores, outliers, par, X, meta, idx): the case with X cut to the points the tests assign; idx = their positions in
    the generator's X (victims: meta["pair"][idx] are their pairs)."""
    if name not in _cases:
        pcores, outliers, par, X, meta = EXTRA[name]() if name in EXTRA else T.build_online(name)
        idx = np.arange(len(X))[SUBSET.get(name, slice(None))]
        _cases[name] = (pcores, outliers, par, np.ascontiguousarray(X[idx]), meta, idx)
    return _cases[name]


def rows_points(name):
    pcores, outliers, _, X = case(name)[:4]
    return (len(pcores) if pcores is not None else 0) + (len(outliers) if outliers is not None else 0), len(X)


def frozen_answers(pcores, outliers, par, X):
    """(uid, path, dist) per point of X, each against a fresh oracle that holds the two lists."""
    from oracle import oracle as O
    n = len(X)
    uid, path, dist = np.empty(n, np.int64), np.empty(n, np.int8), np.empty(n, np.float64)
    for i in range(n):
        o = T.make_oracle(par, pcores, outliers)
        o.online_microcluster_maintenance(X[i:i + 1], 0, reset_param=False, offline=False)
        uid[i], path[i] = o.labels_uid[0], o.paths[0]
        if path[i] == 2:
            uid[i], dist[i] = -1, -1.0
        else:
            t = pcores if path[i] == 0 else outliers
            r = int(np.flatnonzero(t.uid == uid[i])[0])
            dist[i] = O.projected_distance(t.cen[r], t.pref[r], X[i])
    return uid, path, dist


def frozen(name):
    """The referee's (uid, path, dist) for the points of case(name)."""
    if name not in _frozen:
        pcores, outliers, par, X = case(name)[:4]
        _frozen[name] = frozen_answers(pcores, outliers, par, X)
    return _frozen[name]


def sequential(name):
    """(uid, path) of the same points through ONE oracle, one after the other: what an implementation that secretly runs
    the online phase would answer."""
    pcores, outliers, par, X = case(name)[:4]
    o = T.make_oracle(par, pcores, outliers)
    o.online_microcluster_maintenance(X, 0, reset_param=False, offline=False)
    return o.labels_uid.copy(), o.paths.copy()


def same_assign(got, exp, what=""):
    """Bit equality per point of uid and path (and of dist where the library was asked for it); the first differing point
    is named."""
    for key, a, b in zip(("uid", "path", "dist"), got, exp):
        if a is None:
            continue
        diff = T._first_diff(a, b)
        assert diff is None, "%s %s per point (library / referee): %s" % (what, key, diff)
