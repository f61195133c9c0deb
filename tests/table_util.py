"""Injected microcluster tables for the tests of everything after the online phase: the offline PreDeCon phase
(cc_offline), the timestep boundary (cc_decay_downgrade) and the association tracker (cc_assoc_argmin).

Seeded numpy generators build a pcore (and outlier) list directly - centroids, weights, per-dimension variances and
stored preference vectors chosen independently of one another, rows shuffled so that list position says nothing about
geometry - together with the parameter tuple of Handle.set_params.  The same table goes into a _lib.Handle
(inject_bulk) and into the CPU oracle (inject); `same_offline` compares the two offline phases bit for bit and names the
first differing pcore position and key.  Every generator has a structure check that runs on the oracle's output alone
(no GPU): `python tests/table_util.py` runs them all, the GPU tests call them before comparing.
"""
import threading
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "eps_sq delta_sq k beta mu omicron ups_eps ups_eps_sq delta pi")
KEYS = ("cf1", "cf2", "cen", "pref", "w", "id", "uid")


class Table(object):
    """One microcluster list: cf1, cf2, cen, pref [m, d]; w, id, uid [m]."""

    def __init__(self, cen, var, pref, w, id, uid):
        self.cen = np.ascontiguousarray(cen, dtype=np.float64)
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        self.cf1 = self.cen * self.w[:, None]
        self.cf2 = (np.asarray(var, dtype=np.float64) + self.cen * self.cen) * self.w[:, None]
        self.pref = np.ascontiguousarray(np.broadcast_to(pref, self.cen.shape), dtype=np.float64)
        self.id = np.ascontiguousarray(id, dtype=np.int64)
        self.uid = np.ascontiguousarray(uid, dtype=np.int64)

    def __len__(self):
        return len(self.w)

    @property
    def d(self):
        return self.cen.shape[1]

    def columns(self):
        return tuple(getattr(self, k) for k in KEYS)


def _ids(rng, m, first):
    """Distinct creation numbers that are not the list positions."""
    return first + rng.permutation(m).astype(np.int64)


def _table(rng, cen, var, pref, w, first_id=0, first_uid=1_000_000):
    m = len(w)
    return Table(cen, var, pref, w, _ids(rng, m, first_id), _ids(rng, m, first_uid))


# ---- generators ---------------------------------------------------------------------------------------------------

def chains(seed, mp, d, L, step=0.025, shifted=False):
    """Groups of L centroids stepping along one dimension (group g along dimension g % d), groups 50 apart in dimension
    0.  epsilon 0.03, upsilon 2, delta 0.05, k 4, pi = d: with step 0.025 a centroid's eps-neighbourhood holds the two
    next ones on either side, the weighted test (4 * step^2 <= 0.0036) passes for the adjacent ones only and a chain
    merges into one cluster; with step 0.04 the eps test passes for the adjacent ones and the weighted test fails
    (singletons).  Rows are shuffled, then chain 0 gets list positions 0 and mp - 1: its members span the bitmask.
    shifted: the same table translated by 1e6 and scaled by 2^-40 (thresholds scaled with it, variances 0)."""
    rng = np.random.default_rng(seed)
    r = np.arange(mp)
    g, i = r // L, r % L
    n_groups = int(g.max()) + 1
    cen = rng.uniform(0.0, 1.0, (n_groups, d))[g]
    cen[:, 0] += 50.0 * g
    cen[r, g % d] += i * step
    w = rng.uniform(2.0, 10.0, mp)
    var = rng.uniform(0.0, 1e-6, (mp, d))
    eps_sq, delta_sq, ups_eps, delta = 0.03 ** 2, 0.05 ** 2, 2.0 * 0.03, 0.05
    if shifted:
        s = 2.0 ** -40
        cen = (cen + 1e6) * s
        var = np.zeros((mp, d))
        eps_sq, delta_sq, ups_eps, delta = s * s, delta_sq * s ** 4, ups_eps * s, delta * s * s
    perm = rng.permutation(mp)
    pos_of = np.empty(mp, np.int64)
    pos_of[perm] = np.arange(mp)            # row r of the geometric order sits at list position pos_of[r]
    chain0 = np.flatnonzero(g == 0)
    if len(chain0) >= 2:                     # chain 0 takes the two ends of the list
        for row, want in ((chain0[0], 0), (chain0[1], mp - 1)):
            other = perm[want]
            a, b = pos_of[row], pos_of[other]
            perm[a], perm[b] = other, row
            pos_of[row], pos_of[other] = b, a
    t = _table(rng, cen[perm], var[perm], 4.0, w[perm])
    par = Params(eps_sq, delta_sq, 4.0, 0.5, 1.0, 0.1, ups_eps, ups_eps ** 2, delta, d)
    return t, par, dict(kind="chains", L=min(L, mp), group=g[perm], singletons=step > 0.03)


def dense(seed, mp, d):
    """Every pcore within epsilon of every other and weighted-reachable from it: full 64-bit words, mp^2 neighbour
    list entries, one cluster whose merge order is the whole list."""
    rng = np.random.default_rng(seed)
    cen = rng.uniform(0.0, 0.01, (mp, d))
    t = _table(rng, cen, rng.uniform(0.0, 1e-6, (mp, d)), 4.0, rng.uniform(2.0, 10.0, mp))
    return t, Params(0.03 ** 2, 0.05 ** 2, 4.0, 0.5, 1.0, 0.1, 1.0, 1.0, 0.05, d), dict(kind="dense")


def lattice_ties(seed, mp, d, k=4.0):
    """Centroids on a 1/8 grid: groups of ~24 around far-apart group centres, offsets of -2..2 eighths in three
    dimensions.  Every sum is exact whatever its order; ups_eps = 1/2, ups_eps_sq = 1/4 and delta = 1/32 are values the
    three `<=` comparisons of the pair kernels meet exactly (`ties_present` recomputes them in numpy)."""
    rng = np.random.default_rng(seed)
    g = np.arange(mp) // 24
    n_groups = int(g.max()) + 1
    centre = np.zeros((n_groups, d))
    centre[:, 0] = 8.0 * np.arange(n_groups)
    centre += rng.integers(0, 8, (n_groups, d)) / 8.0
    off = np.zeros((mp, d))
    for gi in range(n_groups):
        rows = np.flatnonzero(g == gi)
        act = rng.choice(d, min(d, 3), replace=False)
        off[np.ix_(rows, act)] = rng.integers(-2, 3, (len(rows), len(act))) / 8.0
    cen = centre[g] + off
    perm = rng.permutation(mp)
    t = _table(rng, cen[perm], rng.uniform(0.0, 1e-6, (mp, d)), k, rng.uniform(2.0, 10.0, mp))
    return t, Params(0.03 ** 2, 0.05 ** 2, k, 0.5, 1.0, 0.1, 0.5, 0.25, 1.0 / 32.0, d), dict(kind="ties")


def ties_present(t, par):
    """(pairs with sqrt(acc) == ups_eps, (p, dim) with var == delta, eps-neighbour pairs with dist == ups_eps_sq) of a
    lattice table, recomputed in numpy: all terms are small dyadic numbers, so every sum is exact in any order."""
    cen, d = t.cen, t.d
    diff2 = (cen[:, None, :] - cen[None, :, :]) ** 2
    acc = diff2.sum(axis=2)
    nb = np.sqrt(acc) <= par.ups_eps
    var = (diff2 * nb[:, :, None]).sum(axis=1) / nb.sum(axis=1)[:, None]
    wvec = np.where(var <= par.delta, par.k, 1.0)
    dpq = (diff2 * wvec[:, None, :]).sum(axis=2)
    dist = np.maximum(dpq, dpq.T)
    return int((np.sqrt(acc) == par.ups_eps).sum()), int((var == par.delta).sum()), int((nb & (dist == par.ups_eps_sq)).sum())


def mixed(seed, mp, d, k=4.0, foreign=False):
    """Groups of 1-12 pcores, far apart, fully connected within (eps and weighted): in `n_wide` of the dimensions a
    group's members sit at +-0.5 (neighbourhood variance above delta), in the others they differ by a jitter, so every
    member's PreDeCon pdim is d - n_wide against pi = d - 2.  A group with n_wide >= 2 and a core member becomes one
    cluster of all its members in list order; the others become none.  About 40 % of the rows are not core: weight
    below mu, projected radius above eps_sq, or more than pi stored preference entries above 1 (stored entries are k
    or 1; with `foreign` a few are 2.5, the trace of an earlier k).  Returns what the construction implies: the core
    flags, the clusters, and how often each corner of the ordered expansion occurs."""
    assert d >= 3
    rng = np.random.default_rng(seed)
    pi, mu, a = d - 2, 4.0, 0.5
    sizes = []
    while sum(sizes) < mp:
        sizes.append(int(min(rng.integers(1, 13), mp - sum(sizes))))
    g = np.repeat(np.arange(len(sizes)), sizes)
    n_wide = rng.integers(0, min(3, d) + 1, len(sizes))
    cen = rng.normal(0.0, 1e-3, (mp, d))
    gi = np.arange(len(sizes))
    cen[:, 0] += 10.0 * (gi % 16)[g]
    cen[:, 1] += 10.0 * ((gi // 16) % 16)[g]
    cen[:, 2] += 10.0 * (gi // 256)[g]
    start = 0
    for i, sz in enumerate(sizes):
        if sz == 1:
            n_wide[i] = 0
        for dim in rng.choice(d, n_wide[i], replace=False):
            side = rng.integers(0, 2, sz)
            side[0], side[1] = 0, 1                         # both sides are taken
            cen[start:start + sz, dim] += np.where(side == 1, a, -a)
        start += sz
    core = rng.random(mp) < 0.6
    reason = rng.integers(0, 3, mp)                          # of a non-core row
    w = rng.uniform(4.0, 20.0, mp)
    w[rng.random(mp) < 0.1] = mu                             # `w >= mu` at equality
    w[~core & (reason == 0)] = rng.uniform(1.0, 3.9, int((~core & (reason == 0)).sum()))
    var = rng.uniform(0.0, 1e-4, (mp, d)) / d
    var[~core & (reason == 1)] = 0.02                        # radius >= 0.02 * d / k > eps_sq = 0.01
    pref = np.ones((mp, d))
    for r in range(mp):
        if not core[r] and reason[r] == 2:
            pref[r] = k                                      # d entries above 1 > pi
        else:
            pref[r, rng.choice(d, int(rng.integers(0, pi + 1)), replace=False)] = k
    if foreign:
        rows = rng.choice(mp, max(1, mp // 50), replace=False)
        for r in rows:
            on = np.flatnonzero(pref[r] > 1.0)
            if len(on):
                pref[r, on[0]] = 2.5
    perm = rng.permutation(mp)
    t = _table(rng, cen[perm], var[perm], pref[perm], w[perm])
    g, core = g[perm], core[perm]
    # what the construction implies
    claimed_noise, barren_seeds, queued_noncore = 0, 0, 0
    order = {}
    for pos in range(mp):
        order.setdefault(int(g[pos]), []).append(pos)
    seeds = []
    for grp, members in order.items():
        cores = [p for p in members if core[p]]
        if not cores:
            continue
        if n_wide[grp] >= 2:
            seeds.append((cores[0], members))
            claimed_noise += sum(1 for p in members if not core[p] and p < cores[0])
            queued_noncore += sum(1 for p in members if not core[p] and p > cores[0])
        else:
            barren_seeds += len(cores)
    clusters = [[int(t.id[p]) for p in members] for _, members in sorted(seeds)]
    par = Params(0.01, 0.05 ** 2, k, 0.5, mu, 0.1, 2.0, 4.0, 0.05, pi)
    return t, par, dict(kind="mixed", core=core.astype(np.int8), pdim=(d - n_wide[g]).astype(np.int32),
                        clusters=clusters, claimed_noise=claimed_noise, barren_seeds=barren_seeds,
                        queued_noncore=queued_noncore)


# ---- the two sides --------------------------------------------------------------------------------------------------

def make_oracle(par, pcores=None, outliers=None, lam=1.0):
    """An OracleHDDStream with exactly the parameters of `par` (no dataset-dependent derivation) and the two lists."""
    from oracle import oracle as O
    o = O.OracleHDDStream(dict(epsilon=1.0, upsilon=1.0, delta=0.5, beta=par.beta, k=par.k, **{"lambda": lam}))
    o.__dict__.update(epsilon_squared=par.eps_sq, delta_squared=par.delta_sq, k=par.k, beta=par.beta, mu=par.mu,
                      omicron=par.omicron, upsilon=par.ups_eps, delta=par.delta, pi=par.pi, lambbda=lam)
    assert o.upsilon ** 2 == par.ups_eps_sq  # (_push_params squares it)
    o._push_params()
    for kind, t in ((O.PCORE, pcores), (O.OUTLIER, outliers)):
        if t is not None:
            for r in range(len(t)):
                o.inject(kind, t.cf1[r], t.cf2[r], t.cen[r], t.pref[r], t.w[r], t.id[r], t.uid[r])
    return o


def oracle_lib():
    from oracle import oracle as O
    return O.lib()


def fill_handle(h, par, pcores=None, outliers=None):
    """set_params BEFORE injecting: without parameters every stored entry other than 1 would taint the handle."""
    from chronoclust_amd import _lib
    h.set_params(*par)
    for kind, t in ((_lib.PCORE, pcores), (_lib.OUTLIER, outliers)):
        if t is not None and len(t):
            h.inject_bulk(kind, *t.columns())
    return h


def oracle_offline(o):
    """The oracle's offline phase as (dumps incl. num_core, clusters)."""
    from oracle import oracle as O
    o.offline_clustering()
    info = dict(o.offline_dump)
    info["num_core"] = int(O.lib().co_num_core(o._h))
    return info, o.clusters


def handle_offline(h):
    clusters, info = h.offline(dumps=True)
    info = dict(info)
    info["num_core"] = h.num_core()
    return info, clusters


def _first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return "shapes %r / %r" % (a.shape, b.shape)
    neq = ~((a == b) | ((a != a) & (b != b)))  # (NaN equals NaN here: both sides computed the same thing)
    if not neq.any():
        return None
    at = tuple(int(x) for x in np.argwhere(neq)[0])
    return "first difference at %r (bitmask word %d): %r / %r (%d differ)" % (
        at, at[0] // 64, a[at].item(), b[at].item(), int(neq.sum()))


def same_offline(got, exp, what=""):
    """Bit equality of core, pdim, nn, nw, num_core, the number of clusters, every cluster's members in merge order and
    its w, cf1, cf2, cen, pref.  got / exp: (info, clusters) of handle_offline / oracle_offline."""
    (gi, gc), (ei, ec) = got, exp
    for key in ("core", "pdim", "nn", "nw"):
        diff = _first_diff(gi[key], ei[key])
        assert diff is None, "%s %s per pcore position (library / oracle): %s" % (what, key, diff)
    assert gi["num_core"] == ei["num_core"], "%s num_core %d / %d" % (what, gi["num_core"], ei["num_core"])
    assert len(gc) == len(ec), "%s clusters: %d / %d" % (what, len(gc), len(ec))
    for c, (a, b) in enumerate(zip(gc, ec)):
        am, bm = [int(x) for x in a["members"]], [int(x) for x in b["members"]]
        if am != bm:
            first = next((i for i, (x, y) in enumerate(zip(am, bm)) if x != y), min(len(am), len(bm)))
            raise AssertionError("%s cluster %d: members differ from merge position %d on (%d / %d members)"
                                 % (what, c, first, len(am), len(bm)))
        assert a["w"] == b["w"] or (a["w"] != a["w"] and b["w"] != b["w"]), "%s cluster %d: w %r / %r" % (what, c, a["w"], b["w"])
        for key in ("cf1", "cf2", "cen", "pref"):
            diff = _first_diff(a[key], b[key])
            assert diff is None, "%s cluster %d %s: %s" % (what, c, key, diff)


def same_lists(h, o, what=""):
    """Both lists (order included) and the id counters of a handle against the oracle's, bit for bit."""
    for kind, name in ((0, "pcore"), (1, "outlier")):
        a, b = h.export(kind), o.table(kind)
        for key in ("id", "uid", "w", "cf1", "cf2", "cen", "pref"):
            diff = _first_diff(a[key], b[key])
            assert diff is None, "%s %s list, %s: %s" % (what, name, key, diff)
    assert h.counters() == o.counters, "%s counters %r / %r" % (what, h.counters(), o.counters)


def group_offline(world, par, pcores, device=0):
    """The offline phase of `world` handles of one in-process group (the row-sharded path forced on from the first row),
    one host thread per rank: [(info, clusters)] by rank."""
    from chronoclust_amd import _lib
    hs = [_lib.Handle(device) for _ in range(world)]
    try:
        _lib.comm_init_local(hs)
        results, errors = [None] * world, [None] * world

        def work(rank):
            try:
                hs[rank].set_shard_thresholds(0, 0)
                fill_handle(hs[rank], par, pcores)
                results[rank] = handle_offline(hs[rank])
            except BaseException as e:  # noqa: BLE001 - reported after the join
                errors[rank] = e
                try:
                    hs[rank].comm_destroy()  # the peers must not wait for this rank
                except Exception:
                    pass

        threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        for e in errors:
            if e is not None:
                raise e
        return results
    finally:
        for h in hs:
            h.close()


# ---- structure checks: conditions on the inputs, on the oracle's own output -----------------------------------------

def check_structure(t, par, meta, info, clusters):
    """Asserts that the structure a table exists for is present in the ORACLE's result (no GPU involved)."""
    mp, kind = len(t), meta["kind"]
    pos_of_id = {int(x): p for p, x in enumerate(t.id)}
    sizes = [len(c["members"]) for c in clusters]
    if kind == "chains" and meta["singletons"]:
        assert sizes == [1] * mp and info["nn"].max() == 3 and info["nw"].max() == 1
    elif kind == "chains":
        L = meta["L"]
        big = max(clusters, key=lambda c: len(c["members"]))
        assert len(big["members"]) >= L and info["num_core"] == mp
        pos = np.array([pos_of_id[int(x)] for x in clusters[0]["members"]])  # (position 0 belongs to chain 0)
        assert len(pos) >= L and pos.min() == 0 and (mp < 2 or pos.max() == mp - 1)
        if mp > 4096:
            assert pos.max() // 64 - pos.min() // 64 + 1 > 64 and pos.min() < 4096 <= pos.max()
        if mp >= 5 and L >= 5:
            assert info["nn"].max() == 5 and info["nw"].max() == 3
    elif kind == "dense":
        assert info["nn"].min() == mp and info["nw"].min() == mp and sizes == [mp]
        assert [int(x) for x in clusters[0]["members"]] == [int(x) for x in t.id]
    elif kind == "ties":
        n_eps, n_var, n_w = ties_present(t, par)
        assert n_eps > 0 and n_var > 0 and n_w > 0, (n_eps, n_var, n_w)
        assert len(np.unique(info["nn"])) > 3 and len(np.unique(info["pdim"])) > 1 and max(sizes) > 1
    elif kind == "mixed":
        assert np.array_equal(info["core"], meta["core"]) and np.array_equal(info["pdim"], meta["pdim"])
        share = 1.0 - info["core"].mean()
        assert 0.1 <= share <= 0.9 and (info["pdim"] > par.pi).any() and (info["pdim"] <= par.pi).any()
        assert [[int(x) for x in c["members"]] for c in clusters] == meta["clusters"]
        assert meta["claimed_noise"] > 0 and meta["barren_seeds"] > 0 and meta["queued_noncore"] > 0
    else:
        raise ValueError(kind)


# every offline table of tests/test_offline_tables.py: name -> (generator, arguments).  Sizes around the word (64), the
# batch of 64 words (4 096) and the default sharding threshold (8 192); every compiled width of k_eps_neighbours (4, 8,
# 16, 20, 24, 40, 64, 128, blocked) and its neighbours, each with more than one word.
OFFLINE_TABLES = {
    "chains-1x1": (chains, dict(seed=1, mp=1, d=1, L=1)),
    "chains-63x3": (chains, dict(seed=2, mp=63, d=3, L=7)),
    "chains-64x4": (chains, dict(seed=3, mp=64, d=4, L=8)),
    "chains-65x5": (chains, dict(seed=4, mp=65, d=5, L=13)),
    "chains-4095x8": (chains, dict(seed=5, mp=4095, d=8, L=300)),
    "chains-4096x13": (chains, dict(seed=6, mp=4096, d=13, L=300)),
    "chains-4097x16": (chains, dict(seed=7, mp=4097, d=16, L=300)),
    "chains-8191x17": (chains, dict(seed=8, mp=8191, d=17, L=300)),
    "chains-8192x20": (chains, dict(seed=9, mp=8192, d=20, L=300)),
    "chains-4097x21": (chains, dict(seed=10, mp=4097, d=21, L=64)),
    "chains-8191x24": (chains, dict(seed=11, mp=8191, d=24, L=300)),
    "chains-4097x25": (chains, dict(seed=12, mp=4097, d=25, L=7)),
    "chains-8192x40": (chains, dict(seed=13, mp=8192, d=40, L=300)),
    "chains-4097x41": (chains, dict(seed=14, mp=4097, d=41, L=300)),
    "chains-4097x64": (chains, dict(seed=15, mp=4097, d=64, L=300)),
    "chains-4097x65": (chains, dict(seed=16, mp=4097, d=65, L=300)),
    "chains-4096x128": (chains, dict(seed=17, mp=4096, d=128, L=300)),
    "chains-4097x129": (chains, dict(seed=18, mp=4097, d=129, L=300)),
    "chains-4097x300": (chains, dict(seed=19, mp=4097, d=300, L=300)),
    "chains-24000x20": (chains, dict(seed=20, mp=24000, d=20, L=300)),
    "chains-32768x40": (chains, dict(seed=32, mp=32768, d=40, L=300)),
    "singletons-4097x20": (chains, dict(seed=21, mp=4097, d=20, L=300, step=0.04)),
    "shifted-4097x20": (chains, dict(seed=22, mp=4097, d=20, L=300, shifted=True)),
    "shifted-65x129": (chains, dict(seed=23, mp=65, d=129, L=13, shifted=True)),
    "dense-6001x5": (dense, dict(seed=24, mp=6001, d=5)),
    "ties-300x3": (lattice_ties, dict(seed=25, mp=300, d=3)),
    "ties-500x17": (lattice_ties, dict(seed=26, mp=500, d=17, k=3.0)),
    "ties-200x129": (lattice_ties, dict(seed=27, mp=200, d=129)),
    "mixed-k4-4097x16": (mixed, dict(seed=28, mp=4097, d=16, k=4.0)),
    "mixed-k3-4097x16": (mixed, dict(seed=28, mp=4097, d=16, k=3.0)),
    "mixed-foreign-4097x16": (mixed, dict(seed=28, mp=4097, d=16, k=4.0, foreign=True)),
    "mixed-k4-65x4": (mixed, dict(seed=29, mp=65, d=4, k=4.0)),
    "mixed-k3-8192x40": (mixed, dict(seed=30, mp=8192, d=40, k=3.0)),
    "mixed-foreign-1000x300": (mixed, dict(seed=31, mp=1000, d=300, k=4.0, foreign=True)),
}


def build_table(name):
    gen, kw = OFFLINE_TABLES[name]
    return gen(**kw)


if __name__ == "__main__":  # the structure conditions of every table against the oracle alone (no GPU)
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name in sys.argv[1:] or OFFLINE_TABLES:
        t0 = time.time()
        t, par, meta = build_table(name)
        info, clusters = oracle_offline(make_oracle(par, t))
        check_structure(t, par, meta, info, clusters)
        print("%-26s ok: %5d pcores, %5d core, %5d clusters (largest %d), nn %d..%d, nw %d..%d, %.1f s" % (
            name, len(t), info["num_core"], len(clusters), max([len(c["members"]) for c in clusters] or [0]),
            info["nn"].min(), info["nn"].max(), info["nw"].min(), info["nw"].max(), time.time() - t0))
