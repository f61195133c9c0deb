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


def _run_group(world, work, device=0):
    """`world` handles of one in-process group, work(handle, rank) on one host thread per rank.  A rank that fails leaves the
    group, so that its peers do not wait for it; the first error is raised after the join, the handles closed.  Returns
    (the handles - the caller closes them -, what work returned by rank)."""
    from chronoclust_amd import _lib
    hs = [_lib.Handle(device) for _ in range(world)]
    try:
        _lib.comm_init_local(hs)
        results, errors = [None] * world, [None] * world

        def run(rank):
            try:
                results[rank] = work(hs[rank], rank)
            except BaseException as e:  # noqa: BLE001 - reported after the join
                errors[rank] = e
                try:
                    hs[rank].comm_destroy()  # the peers must not wait for this rank
                except Exception:
                    pass

        threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        for e in errors:
            if e is not None:
                raise e
        return hs, results
    except BaseException:
        for h in hs:
            h.close()
        raise


def group_offline(world, par, pcores, device=0):
    """The offline phase of `world` handles of one in-process group (the row-sharded path forced on from the first row),
    one host thread per rank: [(info, clusters)] by rank."""
    def work(h, rank):
        h.set_shard_thresholds(0, 0)
        fill_handle(h, par, pcores)
        return handle_offline(h)

    hs, results = _run_group(world, work, device)
    for h in hs:
        h.close()
    return results


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


# ---- the online phase on injected tables ------------------------------------------------------------------------------
#
# A streamed table always agrees with itself: stored preference entries are k or 1 as the row's CF1 / CF2 and the current k
# say, the table is never larger than the points seen, and list position follows creation time.  The generators below
# build both lists directly, give them to handle and oracle alike and send points through
#     make_oracle(par, pcores, outliers).online_microcluster_maintenance(X, 0, reset_param=False, offline=False)
# (no decay, no parameter derivation) on one side and fill_handle + Handle.online(X) on the other.  Each returns
# (pcores, outliers, params, X, meta); `check_online` asserts on the ORACLE's result that what the case exists for happened.

def _sites(rng, n, d, sep, lo=0.1, hi=0.9):
    """n points of [lo, hi)^d.  Up to 1 500 of them are drawn one at a time, pairwise at least `sep` apart; larger sets
    are only used where d makes a closer pair improbable (the structure checks notice one)."""
    if n > 1500:
        return rng.uniform(lo, hi, (n, d))
    out = np.empty((n, d))
    i = tries = 0
    while i < n:
        c = rng.uniform(lo, hi, d)
        tries += 1
        assert tries < 200 * n + 1000, "no room for %d sites %g apart in %d dimensions" % (n, sep, d)
        if i == 0 or ((out[:i] - c) ** 2).sum(axis=1).min() >= sep * sep:
            out[i] = c
            i += 1
    return out


def _unit(rng, n, d, first=None):
    """n random unit vectors of d dimensions, zero beyond the first `first` of them."""
    u = np.zeros((n, d))
    f = d if first is None else min(d, first)
    u[:, :f] = rng.normal(size=(n, f))
    return u / np.sqrt((u * u).sum(axis=1))[:, None]


def _outlier_table(rng, cen, var, pref, w, first=2_000_000):
    ids = _ids(rng, len(w), first)
    return Table(cen, var, pref, w, ids, ids)            # (an outlier's id is its uid)


def tentative(t, rows, x, par):
    """(pdim, projected radius) of rows `rows` of a table after the tentative add of the points x [len(rows), d]: the
    reference's expressions (cf2 / w - (cf1 / w)^2, entry k where that is <= delta_sq) in numpy."""
    w = (t.w[rows] + 1.0)[:, None]
    var = (t.cf2[rows] + x * x) / w - ((t.cf1[rows] + x) / w) ** 2
    pref = np.where(var <= par.delta_sq, par.k, 1.0)
    return (pref != 1.0).sum(axis=1), (var / pref).sum(axis=1)


def victims(seed, pairs, d, k=4.0, stored=None, on_outliers=False, filt=False, D=0.05, points=None):
    """Taint: pairs of rows (R, R2), the pairs at least 4 D apart, one point p per pair.  R holds `stored` (>= 256 max(k, 1),
    by default 4 096 max(k, 1)) in every stored entry and lies at Euclidean distance D from p, the offset within the first
    eight dimensions (all of them part of every prefix test); R2 holds entries of 1 and lies at distance E, E^2 = 4 D^2 /
    stored.  The reference's distances are D^2 / stored to R and 4 D^2 / stored to R2: R wins.  A bound that takes
    min(1, 1 / k) for the smallest weight of a dimension puts R at D^2 / max(k, 1) or more - beyond 16 x either distance.
    Coordinates stay within [0, 1) and D is 0.05, so that half-precision prefixes resolve the offset (2^-11 of the range a
    coordinate).  A join recomputes the entries with the current k, so every R is hit once.  Weights 10, variances up to
    1e-8, eps 0.05: the tentative radius is D^2 10 / 121 at most.
    on_outliers: the rows on the outlier list (beta mu = 2: every join promotes), a few far pcores beside them.
    filt: pi = d - 3; R and R2 carry three dimensions of variance 4 delta_sq (delta_sq 4e-5 keeps the radius below eps_sq),
    and a third row R3 per pair - entries 1, every variance tiny, E / 4 from p - is nearer than R and rejected by the
    filter (its tentative pdim is d).  points: only so many of the pairs get their point."""
    rng = np.random.default_rng(seed)
    stored = float(stored) if stored else 4096.0 * max(k, 1.0)
    assert stored >= 256.0 * max(k, 1.0)
    nw = 3 if filt else 0
    delta_sq = 4e-5 if filt else 0.05 ** 2
    n_decoy = max(1, pairs // 8) if on_outliers else 0
    sites = _sites(rng, pairs + n_decoy, d, 4.0 * D)
    cR = sites[:pairs]
    X = cR + D * _unit(rng, pairs, d, first=8)
    E = 2.0 * D / np.sqrt(stored)
    cens = [cR, X + E * _unit(rng, pairs, d)] + ([X + 0.25 * E * _unit(rng, pairs, d)] if filt else [])
    prefs = [np.full((pairs, d), stored), np.ones((pairs, d))] + ([np.ones((pairs, d))] if filt else [])
    var = rng.uniform(0.0, 1e-8, (len(cens) * pairs, d))
    for r in range(2 * pairs if filt else 0):
        var[r, rng.choice(d, nw, replace=False)] = 4.0 * delta_sq
    m = len(cens) * pairs
    perm = rng.permutation(m)
    pos_of = np.empty(m, np.int64)
    pos_of[perm] = np.arange(m)
    cen, pref, var = np.concatenate(cens)[perm], np.concatenate(prefs)[perm], var[perm]
    w = np.full(m, 10.0)
    if on_outliers:
        rows = _outlier_table(rng, cen, var, pref, w)
        pcores = _table(rng, sites[pairs:], rng.uniform(0.0, 1e-8, (n_decoy, d)),
                        np.where(rng.random((n_decoy, d)) < 0.5, k, 1.0), np.full(n_decoy, 10.0))
        outliers = rows
    else:
        rows = _table(rng, cen, var, pref, w)
        pcores, outliers = rows, None
    order = rng.permutation(pairs)[:points]               # the points in an order of their own
    par = Params(0.05 ** 2, delta_sq, k, 0.5, 4.0, 0.1, 0.5, 0.25, 0.05, d - nw)
    meta = dict(kind="victims", tainted=True, on_outliers=on_outliers, filt=filt, rows=rows, pair=order,
                R=pos_of[:pairs], R2=pos_of[pairs:2 * pairs], R3=pos_of[2 * pairs:] if filt else None)
    return pcores, outliers, par, np.ascontiguousarray(X[order]), meta


def victims_by_set_params(seed, pairs, d, k=4.0, k_first=4096.0, D=0.05):
    """The same pairs with nothing injected: a first call with k = k_first (a power of two, >= 256 max(k, 1)) builds the
    rows from points - per pair ten points c2 +- v (|v_i| = 1e-4 > delta = 5e-5: entries of 1), then forty points on cR
    (variance 0: entries of k_first) -, then k is lowered on handle and oracle alike (meta["first"] holds the first call's
    parameters and points) and the victim points follow.  eps_sq is 1e-4: a point D from a row of weight 10 fails its radius
    test (D^2 10 / 121 = 2.1e-4), which keeps R's points out of R2; a point D from a row of weight 40 passes
    (D^2 40 / 1 681 = 5.9e-5), which lets the victim join R.  beta mu = 4: both rows are pcores after four points."""
    rng = np.random.default_rng(seed)
    assert k_first >= 256.0 * max(k, 1.0)
    cR = _sites(rng, pairs, d, 4.0 * D)
    X = cR + D * _unit(rng, pairs, d, first=8)
    c2 = X + 2.0 * D / np.sqrt(k_first) * _unit(rng, pairs, d)
    v = 1e-4 * np.where(rng.random((pairs, d)) < 0.5, -1.0, 1.0)
    sign = np.tile(np.array([1.0, -1.0]), 5)
    pts2 = (c2[:, None, :] + sign[None, :, None] * v[:, None, :]).reshape(pairs * 10, d)
    own2 = np.repeat(np.arange(pairs), 10)
    o2 = rng.permutation(len(pts2))
    ptsR, ownR = np.repeat(cR, 40, axis=0), np.repeat(np.arange(pairs), 40)
    oR = rng.permutation(len(ptsR))
    X0 = np.ascontiguousarray(np.concatenate([pts2[o2], ptsR[oR]]))
    order = rng.permutation(pairs)
    first = Params(1e-4, 2.5e-9, k_first, 0.5, 8.0, 0.1, 0.5, 0.25, 0.05, d)
    meta = dict(kind="victims-set-params", tainted=True, first=(first, X0), pair=order, k_first=k_first,
                built_R2=(np.arange(len(o2)), own2[o2]), built_R=(len(o2) + np.arange(len(oR)), ownR[oR]))
    return None, None, first._replace(k=k), np.ascontiguousarray(X[order]), meta


def stale(seed, m_p, m_o, d, n, k=4.0, filt=False, clean=False):
    """General tables whose stored preference entries say nothing about their variances: k or 1 at random, in one row
    in twelve a few entries between 1 and k, in another twelfth a few below both (not with `clean`: entries of k or 1
    only - the handle stays untainted and takes the scans of the common case).  Rows in groups of about four (jitter 0.02
    around centres in [0.1, 0.9)^d), pcore weights 4 .. 40, outlier weights 1 .. 3 with a third at beta mu - 1 = 3 exactly:
    the first join promotes them AT w == beta mu.  filt: pi = d - 2, rows carry 0 .. 4 dimensions of variance 4 delta_sq.
    Points: near pcore centroids, near outlier centroids (half of them near those of weight 3), near pcores that hold
    exactly pi entries above 1, and anywhere in the box (new outliers)."""
    rng = np.random.default_rng(seed)
    pi = d - 2 if filt else d
    delta_sq = 1e-5 if filt else 0.05 ** 2
    beta, mu = 0.5, 8.0
    lo, hi = min(1.0, k), max(1.0, k)

    def rows(m, first_group):
        g = first_group + np.arange(m) // 4
        cen = rng.uniform(0.1, 0.9, (int(g.max()) + 1 if m else 0, d))[g - first_group] + rng.normal(0.0, 0.02, (m, d))
        var = rng.uniform(0.0, 1e-6, (m, d))
        pref = np.where(rng.random((m, d)) < rng.random((m, 1)), k, 1.0)
        for r in range(m):
            if filt:
                var[r, rng.choice(d, int(rng.integers(0, 5)), replace=False)] = 4.0 * delta_sq
            how = int(rng.integers(0, 12))
            if not clean and how < 2:
                at = rng.choice(d, min(d, 3), replace=False)
                pref[r, at] = rng.uniform(lo, hi, len(at)) if how == 0 else 0.5 * lo
        return cen, var, pref

    cen, var, pref = rows(m_p, 0)
    exact = np.zeros(m_p, bool)
    exact[rng.random(m_p) < 0.1] = True                    # exactly pi stored entries above 1
    for r in np.flatnonzero(exact):
        pref[r] = 1.0
        pref[r, rng.choice(d, pi, replace=False)] = k if k > 1.0 else 2.0
    if clean:
        exact &= k > 1.0
        pref[(pref != 1.0) & (pref != k)] = k
    pcores = _table(rng, cen, var, pref, rng.uniform(4.0, 40.0, m_p)) if m_p else None
    cen_o, var_o, pref_o = rows(m_o, m_p // 4 + 1)
    w_o = np.where(rng.random(m_o) < 0.33, beta * mu - 1.0, rng.uniform(1.0, 3.0, m_o))
    outliers = _outlier_table(rng, cen_o, var_o, pref_o, w_o) if m_o else None
    at_eq = np.flatnonzero(w_o == beta * mu - 1.0)
    kinds = rng.choice(4, n, p=[0.4, 0.3, 0.15, 0.15])
    X = rng.uniform(0.1, 0.9, (n, d))
    for i in range(n):
        src = None
        if kinds[i] == 0 and m_p:
            src = cen[rng.integers(0, m_p)]
        elif kinds[i] == 1 and m_o:
            src = cen_o[rng.choice(at_eq)] if len(at_eq) and rng.random() < 0.5 else cen_o[rng.integers(0, m_o)]
        elif kinds[i] == 2 and exact.any():
            src = cen[rng.choice(np.flatnonzero(exact))]
        if src is not None:
            X[i] = src + rng.normal(0.0, 0.003, d)
    par = Params(0.05 ** 2, delta_sq, k, beta, mu, 0.1, 0.5, 0.25, 0.05, pi)
    tainted = not clean
    meta = dict(kind="stale", tainted=tainted, full=m_p >= 31 and m_o >= 31 and n >= 127,
                eq_uids=outliers.uid[at_eq] if m_o else np.zeros(0, np.int64))
    return pcores, outliers, par, np.ascontiguousarray(X), meta


def lattice(seed, m_p, m_o, d, n):
    """Centroids on a 1/8 grid, points on a 1/16 grid, weights 3 or 7 (w + 1 a power of two), variances 0, entries of k = 4 or
    1, thresholds dyadic (eps_sq 3/256, delta_sq 1/16, beta mu 8): every sum is exact in any order, so equal distances ARE
    equal.  Groups of about 24 rows around centres 8 apart in dimension 0, offsets of -2 .. 2 eighths in three dimensions
    (rows of one group may coincide).  Planted on rows that stand alone (4 apart in dimension 1, no group near them):
      copies   one row at pcore-list positions 0, 31, 32, 33 and the last (those the list has), another on the outlier list
               alike; points on its centroid and 1/16 beside it: the first copy in list order takes them all;
      equal    rows of weight 3 with every entry k and a point at c + 1/2 e_1: tentative variance 3/64 (<= delta_sq), radius
               3/256 == eps_sq, accepted;
      beyond   the same with the point at c + 9/16 e_1: radius 243/16384, rejected - a new outlier.
    The other points: a row's centroid plus -2 .. 2 sixteenths in up to three dimensions (midway between two rows of a group:
    an exact tie), and a few far from everything.  Outliers of weight 7 are promoted at w + 1 == beta mu."""
    assert d >= 3
    rng = np.random.default_rng(seed)
    k, eps_sq, delta_sq, beta, mu = 4.0, 3.0 / 256.0, 1.0 / 16.0, 0.5, 16.0

    def general(m, base):
        g = np.arange(m) // 24
        ng = int(g.max()) + 1 if m else 0
        centre = np.zeros((ng, d))
        centre[:, 0] = base + 8.0 * np.arange(ng)
        centre += rng.integers(0, 8, (ng, d)) / 8.0
        off = np.zeros((m, d))
        for gi in range(ng):
            r = np.flatnonzero(g == gi)
            act = rng.choice(d, 3, replace=False)
            off[np.ix_(r, act)] = rng.integers(-2, 3, (len(r), 3)) / 8.0
        return centre[g] + off, np.where(rng.random((m, d)) < 0.5, k, 1.0), rng.choice([3.0, 7.0], m)

    def alone(j, row):                                     # centroid of planted row j of list `row` (0 pcores, 1 outliers)
        c = np.zeros(d)
        c[0], c[1] = -16.0 - 8.0 * row, 4.0 * j
        return c

    def build(m, row, n_eq):
        """A list of m rows: copies at 0, 31, 32, 33, m - 1, then n_eq `equal` and n_eq `beyond` rows at random other
        positions, general rows elsewhere."""
        copy_at = sorted({p for p in (0, 31, 32, 33, m - 1) if 0 <= p < m})
        free = np.array([p for p in rng.permutation(m) if p not in copy_at], np.int64)
        n_eq = min(n_eq, len(free) // 2)
        eq_at, be_at = free[:n_eq], free[n_eq:2 * n_eq]
        cen, pref, w = general(m, 0.0 if row == 0 else 4096.0)
        for p in copy_at:
            cen[p], pref[p], w[p] = alone(0, row), np.where(np.arange(d) % 2 == 0, k, 1.0), 3.0
        for j, p in enumerate(np.concatenate([eq_at, be_at])):
            cen[p], pref[p], w[p] = alone(1 + j, row), k, 3.0
        return cen, pref, w, copy_at, eq_at, be_at

    cen, pref, w, copy_p, eq_at, be_at = build(m_p, 0, 4)
    pcores = _table(rng, cen, 0.0, pref, w) if m_p else None
    cen_o, pref_o, w_o, copy_o, _, _ = build(m_o, 1, 0)
    outliers = _outlier_table(rng, cen_o, 0.0, pref_o, w_o) if m_o else None
    e1 = np.zeros(d)
    e1[1] = 1.0                                            # (dimension 1: "e_1" counting from 0)
    pts, tag = [], []

    def add(x, t):
        pts.append(x)
        tag.append(t)

    for c_at, cc, t in ((copy_p, cen, "copy_p"), (copy_o, cen_o, "copy_o")):
        if c_at:
            for x in (cc[0], cc[0], cc[0] + e1 / 16.0, cc[0] + e1 / 16.0, cc[0] + e1 / 16.0):
                add(x, t)
    for p in eq_at:
        add(cen[p] + e1 / 2.0, "equal")
    for p in be_at:
        add(cen[p] + 9.0 * e1 / 16.0, "beyond")
    both = np.concatenate([cen.reshape(-1, d), cen_o.reshape(-1, d)])
    taken = set(copy_p) | set(int(p) for p in eq_at) | set(int(p) for p in be_at) | set(m_p + p for p in copy_o)
    pool = np.array([r for r in range(len(both)) if r not in taken], np.int64)
    while len(pts) < n:
        if len(pool) == 0 or rng.random() < 0.05:
            x = np.zeros(d)
            x[0], x[2] = -4096.0 - 64.0 * len(pts), 1.0 / 16.0    # far from everything, and from one another
            add(x, "far")
        else:
            x = both[rng.choice(pool)].copy()
            at = rng.choice(d, int(rng.integers(0, 4)), replace=False)
            x[at] += rng.integers(-2, 3, len(at)) / 16.0
            add(x, "near")
    pts, tag0 = np.array(pts), np.array(tag)
    order = rng.permutation(len(pts))
    X, tag = pts[order], tag0[order]
    for t in ("copy_p", "copy_o"):                         # (these keep their order: a point beside the centroid moves it)
        X[tag == t] = pts[tag0 == t]
    par = Params(eps_sq, delta_sq, k, beta, mu, 0.1, 0.5, 0.25, 1.0 / 32.0, d)
    meta = dict(kind="lattice", tainted=False, tag=tag, eq_at=eq_at, be_at=be_at,
                first_copy=(int(pcores.uid[0]) if copy_p else None, int(outliers.uid[0]) if copy_o else None))
    return pcores, outliers, par, np.ascontiguousarray(X), meta


def lattice_present(pcores, par, X, meta):
    """(points whose smallest distance to the injected pcores is shared by two or more rows, `equal` points whose tentative
    radius == eps_sq, `beyond` points whose radius is above it) recomputed in numpy - dyadic terms, exact in any order."""
    ties = 0
    near = np.flatnonzero(meta["tag"] == "near")[:256]
    for i in near:
        dist = ((X[i] - pcores.cen) ** 2 / pcores.pref).sum(axis=1)
        ties += int((dist == dist.min()).sum() > 1)
    eq_pts, be_pts = X[meta["tag"] == "equal"], X[meta["tag"] == "beyond"]

    def radius(pts, rows):                                 # of the planted row each point belongs to (same e_1 line)
        out = []
        for x in pts:
            r = [p for p in rows if pcores.cen[p][0] == x[0] and pcores.cen[p][1] <= x[1] < pcores.cen[p][1] + 1.0]
            out.append(tentative(pcores, np.array(r[:1]), x[None, :], par)[1][0])
        return np.array(out)

    return ties, int((radius(eq_pts, meta["eq_at"]) == par.eps_sq).sum()), int((radius(be_pts, meta["be_at"]) > par.eps_sq).sum())


# ---- the two sides of an online case ------------------------------------------------------------------------------------

def oracle_online(case):
    """The oracle's side of a case: dict(o=the oracle afterwards, uid, path; first=(uid, path) and mid=the pcore list after
    the first call where the case has one)."""
    pcores, outliers, par, X, meta = case
    res = {}
    if "first" in meta:
        par0, X0 = meta["first"]
        o = make_oracle(par0)
        o.online_microcluster_maintenance(X0, 0, reset_param=False, offline=False)
        res["first"] = (o.labels_uid.copy(), o.paths.copy())
        res["mid"] = o.table(0)
        o.__dict__.update(epsilon_squared=par.eps_sq, delta_squared=par.delta_sq, k=par.k, beta=par.beta, mu=par.mu,
                          omicron=par.omicron, upsilon=par.ups_eps, delta=par.delta, pi=par.pi)
    else:
        o = make_oracle(par, pcores, outliers)
    o.online_microcluster_maintenance(X, 0, reset_param=False, offline=False)
    res.update(o=o, uid=o.labels_uid.copy(), path=o.paths.copy())
    return res


def handle_online(h, case):
    """The library's side on a handle that holds nothing: (uid, path) of the case's points, and of the first call's."""
    pcores, outliers, par, X, meta = case
    first = None
    if "first" in meta:
        par0, X0 = meta["first"]
        h.set_params(*par0)
        first = h.online(X0)
        h.set_params(*par)
    else:
        fill_handle(h, par, pcores, outliers)
    return h.online(X), first


def same_online(h, labels, exp, what=""):
    """Bit equality of uid and path per point (the first differing point is named), of both lists and of the id counters.
    labels: what handle_online returned; exp: what oracle_online returned."""
    (uid, path), first = labels
    pairs = [("", uid, path, exp["uid"], exp["path"])]
    if first is not None:
        pairs.insert(0, ("first call: ", first[0], first[1]) + tuple(exp["first"]))
    for pre, gu, gp, eu, ep in pairs:
        for key, a, b in (("uid", gu, eu), ("path", gp, ep)):
            diff = _first_diff(a, b)
            assert diff is None, "%s %s%s per point (library / oracle): %s" % (what, pre, key, diff)
    same_lists(h, exp["o"], what)


def group_online(world, case, device=0, thresholds=(0, 0), tuning=None):
    """The case on `world` handles of one in-process group, one host thread per rank; every split forced on from the first
    row unless `thresholds` says otherwise (None: the library's defaults).  Returns the handles (the caller closes them),
    their labels and their statistics by rank."""
    def work(h, rank):
        if thresholds is not None:
            h.set_shard_thresholds(*thresholds)
        if tuning:
            h.set_tuning(**tuning)
        return handle_online(h, case)

    hs, labels = _run_group(world, work, device)
    return hs, labels, [h.stats() for h in hs]


def check_online(case, res):
    """Asserts on the ORACLE's result that the case holds what it exists for (no GPU involved)."""
    pcores, outliers, par, X, meta = case
    uid, path, kind = res["uid"], res["path"], meta["kind"]
    if kind == "victims":
        t = meta["rows"]
        want = 5 if meta["on_outliers"] else 0
        assert (path == want).all(), "paths %r" % np.unique(path)
        assert np.array_equal(uid, t.uid[meta["R"][meta["pair"]]]), "%d points not absorbed by their R" % int(
            (uid != t.uid[meta["R"][meta["pair"]]]).sum())
        if meta["filt"]:
            r, r2, r3 = (meta[key][meta["pair"]] for key in ("R", "R2", "R3"))
            assert (tentative(t, r3, X, par)[0] > par.pi).all()                     # rejected ...
            assert (tentative(t, r, X, par)[0] <= par.pi).all() and (tentative(t, r2, X, par)[0] <= par.pi).all()
            near = ((X - t.cen[r3]) ** 2 / t.pref[r3]).sum(axis=1)
            assert (near < ((X - t.cen[r]) ** 2 / t.pref[r]).sum(axis=1)).all()      # ... though nearer than R
    elif kind == "victims-set-params":
        fu, fp = res["first"]
        pairs = len(X)
        uid_of = {}
        for name in ("built_R", "built_R2"):
            at, own = meta[name]
            per = [np.unique(fu[at[own == p]]) for p in range(pairs)]
            assert all(len(u) == 1 for u in per), "%s: a pair's points went to several rows" % name
            uid_of[name] = np.array([u[0] for u in per])
        mid = res["mid"]
        row_of = {int(u): i for i, u in enumerate(mid["uid"])}
        assert len(mid["uid"]) == 2 * pairs
        for p in range(pairs):
            a, b = row_of[int(uid_of["built_R"][p])], row_of[int(uid_of["built_R2"][p])]
            assert (mid["pref"][a] == meta["k_first"]).all() and mid["w"][a] == 40.0
            assert (mid["pref"][b] == 1.0).all() and mid["w"][b] == 10.0
        assert (path == 0).all() and np.array_equal(uid, uid_of["built_R"][meta["pair"]])
    elif kind == "stale":
        if meta["full"]:
            seen = set(int(x) for x in np.unique(path))
            assert {0, 1, 5, 2} <= seen, "paths %r" % sorted(seen)
            first_join = {}
            for i in range(len(uid)):
                first_join.setdefault(int(uid[i]), int(path[i]))
            at_eq = [first_join[int(u)] for u in meta["eq_uids"] if int(u) in first_join]
            assert 5 in at_eq, "no outlier of weight beta mu - 1 was promoted by its first join"
    elif kind == "lattice":
        tag = meta["tag"]
        fp, fo = meta["first_copy"]
        if fp is not None and (tag == "copy_p").any():
            assert (uid[tag == "copy_p"] == fp).all() and (path[tag == "copy_p"] == 0).all()
        if fo is not None and (tag == "copy_o").any():
            assert (uid[tag == "copy_o"] == fo).all() and ((path[tag == "copy_o"] & 3) == 1).all()
        if pcores is not None and len(pcores) >= 64 and len(X) >= 127:
            ties, n_eq, n_be = lattice_present(pcores, par, X, meta)
            assert ties > 0 and n_eq > 0 and n_be > 0, (ties, n_eq, n_be)
            assert n_eq == int((tag == "equal").sum()) and n_be == int((tag == "beyond").sum())
            assert (path[tag == "equal"] == 0).all() and sorted(uid[tag == "equal"]) == sorted(pcores.uid[meta["eq_at"]])
            assert (path[tag == "beyond"] == 2).all() and (path[tag == "far"] == 2).all()
            if outliers is not None and len(outliers) >= 64:
                assert (path == 5).any()
    elif kind == "arrivals":                                   # designed arrivals: tests/arrival_util.py
        import arrival_util
        arrival_util.check_arrivals(case, res)
    elif kind == "seq-edge":                                   # the sequential kernels' capacity and hand-over edges: tests/seq_edge_util.py
        import seq_edge_util
        seq_edge_util.check_seq_edge(case, res)
    else:
        raise ValueError(kind)


# every injected table of tests/test_online_tables.py: name -> (generator, arguments).  Row counts around the point tile and
# wave (31 .. 33, 127 .. 129), one list empty, up to 4 096 rows; 1 to 2 048 points; every width at which the online phase
# takes another kernel (3: k_seq_r; 5, 8: k_scan pads for itself; 13: padded rows; 14 .. 64: the ladder; 80, 200: k_seq_g and
# its wide form).  The tables of 9 999 rows and more select forms by table size (see the tests that use them).
# (This set is recorded by tests/golden/surface/online.npz and stays as it is.  Inputs designed for the sequential kernels' OWN
# constants - k_seq_r's slots, k_seq's image and chunk, k_seq_g's stride, the host's chunk of 8 192 points - and the exact share of
# each kernel: tests/seq_edge_util.py, SEQ_EDGE_CASES.)
ONLINE_TABLES = {
    "victims-k4-16x14": (victims, dict(seed=101, pairs=16, d=14)),
    "victims-k4-300x16": (victims, dict(seed=102, pairs=300, d=16)),
    "victims-k4-600x20": (victims, dict(seed=103, pairs=600, d=20)),
    "victims-k4-1000x32": (victims, dict(seed=104, pairs=1000, d=32)),
    "victims-k4-2048x40": (victims, dict(seed=105, pairs=2048, d=40)),
    "victims-k3-600x20": (victims, dict(seed=106, pairs=600, d=20, k=3.0)),
    "victims-k0.5-600x20": (victims, dict(seed=107, pairs=600, d=20, k=0.5)),
    "victims-k3-200x14": (victims, dict(seed=108, pairs=200, d=14, k=3.0, stored=768.0)),
    "victims-outliers-600x20": (victims, dict(seed=109, pairs=600, d=20, on_outliers=True)),
    "victims-outliers-k3-500x40": (victims, dict(seed=110, pairs=500, d=40, k=3.0, on_outliers=True)),
    "victims-filter-600x20": (victims, dict(seed=111, pairs=600, d=20, filt=True)),
    "victims-filter-k3-300x32": (victims, dict(seed=112, pairs=300, d=32, k=3.0, filt=True)),
    "victims-k4-8x3": (victims, dict(seed=113, pairs=8, d=3)),
    "victims-k4-12x5": (victims, dict(seed=114, pairs=12, d=5)),
    "victims-k4-40x8": (victims, dict(seed=115, pairs=40, d=8)),
    "victims-k4-64x13": (victims, dict(seed=116, pairs=64, d=13)),
    "victims-k4-200x64": (victims, dict(seed=117, pairs=200, d=64)),
    "victims-k4-100x80": (victims, dict(seed=118, pairs=100, d=80)),
    "victims-k4-50x200": (victims, dict(seed=119, pairs=50, d=200)),
    "victims-set-params-200x20": (victims_by_set_params, dict(seed=120, pairs=200, d=20)),
    "victims-set-params-k3-100x14": (victims_by_set_params, dict(seed=121, pairs=100, d=14, k=3.0)),
    "victims-k4-10000x20": (victims, dict(seed=122, pairs=10000, d=20, points=2048)),
    "stale-1+0x3": (stale, dict(seed=201, m_p=1, m_o=0, d=3, n=1)),
    "stale-31+33x5": (stale, dict(seed=202, m_p=31, m_o=33, d=5, n=127)),
    "stale-32+0x8": (stale, dict(seed=203, m_p=32, m_o=0, d=8, n=128)),
    "stale-0+129x13": (stale, dict(seed=204, m_p=0, m_o=129, d=13, n=129)),
    "stale-127+128x14": (stale, dict(seed=205, m_p=127, m_o=128, d=14, n=500, filt=True)),
    "stale-1000+500x16": (stale, dict(seed=206, m_p=1000, m_o=500, d=16, n=1000, k=3.0)),
    "stale-3000+1096x20": (stale, dict(seed=207, m_p=3000, m_o=1096, d=20, n=2048)),
    "stale-filter-2000+1000x20": (stale, dict(seed=208, m_p=2000, m_o=1000, d=20, n=2048, filt=True)),
    "stale-k0.5-600x32": (stale, dict(seed=209, m_p=400, m_o=200, d=32, n=700, k=0.5)),
    "stale-filter-1500x40": (stale, dict(seed=210, m_p=1000, m_o=500, d=40, n=1000, k=3.0, filt=True)),
    "stale-600x64": (stale, dict(seed=211, m_p=400, m_o=200, d=64, n=600)),
    "stale-300x80": (stale, dict(seed=212, m_p=200, m_o=100, d=80, n=300)),
    "stale-filter-150x200": (stale, dict(seed=213, m_p=100, m_o=50, d=200, n=200, filt=True)),
    "clean-2000+1000x20": (stale, dict(seed=214, m_p=2000, m_o=1000, d=20, n=2048, clean=True)),
    "clean-filter-1000+500x14": (stale, dict(seed=215, m_p=1000, m_o=500, d=14, n=1000, clean=True, filt=True)),
    "clean-9999x20": (stale, dict(seed=216, m_p=6999, m_o=3000, d=20, n=1024, clean=True)),
    "clean-10000x20": (stale, dict(seed=216, m_p=7000, m_o=3000, d=20, n=1024, clean=True)),
    "clean-10001x20": (stale, dict(seed=216, m_p=7001, m_o=3000, d=20, n=1024, clean=True)),
    "clean-19999x20": (stale, dict(seed=217, m_p=14999, m_o=5000, d=20, n=1024, clean=True)),
    "clean-20000x20": (stale, dict(seed=217, m_p=15000, m_o=5000, d=20, n=1024, clean=True)),
    "lattice-33+33x3": (lattice, dict(seed=301, m_p=33, m_o=33, d=3, n=127)),
    "lattice-64+40x5": (lattice, dict(seed=312, m_p=64, m_o=40, d=5, n=200)),
    "lattice-128+127x8": (lattice, dict(seed=302, m_p=128, m_o=127, d=8, n=300)),
    "lattice-129+64x13": (lattice, dict(seed=303, m_p=129, m_o=64, d=13, n=300)),
    "lattice-1000+500x14": (lattice, dict(seed=304, m_p=1000, m_o=500, d=14, n=1000)),
    "lattice-300+150x16": (lattice, dict(seed=310, m_p=300, m_o=150, d=16, n=400)),
    "lattice-3000+1096x20": (lattice, dict(seed=305, m_p=3000, m_o=1096, d=20, n=2048)),
    "lattice-500+250x32": (lattice, dict(seed=311, m_p=500, m_o=250, d=32, n=600)),
    "lattice-1000+500x40": (lattice, dict(seed=306, m_p=1000, m_o=500, d=40, n=1000)),
    "lattice-400+200x64": (lattice, dict(seed=307, m_p=400, m_o=200, d=64, n=500)),
    "lattice-200+100x80": (lattice, dict(seed=308, m_p=200, m_o=100, d=80, n=300)),
    "lattice-100+64x200": (lattice, dict(seed=313, m_p=100, m_o=64, d=200, n=200)),
    "lattice-7000+3000x20": (lattice, dict(seed=309, m_p=7000, m_o=3000, d=20, n=1024)),
}


def build_online(name):
    gen, kw = ONLINE_TABLES[name]
    return gen(**kw)


# ---- the relaxed multi-GPU mode on injected tables ----------------------------------------------------------------------
#
# Cases for tests/relaxed_model.py (the CPU model of cc_comm_set_relaxed) and tests/test_relaxed_model.py (the library against
# it): (pcores, outliers, params, X, meta) as above; meta carries `world` and `minibatch`, the group the points were laid out
# for - X is world blocks of ceil(n / world) points, block r being rank r's shard.  `check_relaxed` asserts on the MODEL's
# result that what a case exists for happened.

def _lattice_sites(rng, n, d, spacing=0.6):
    """n distinct sites of a grid of the given spacing in the first min(d, 8) dimensions (the further dimensions uniform in
    [0.1, 0.9)), in random order, each moved by up to a thousandth of the spacing: `spacing` apart or more.  At 0.6 a row of
    weight up to 140 refuses a point of the next site (tentative variance 0.36 w / (w + 1)^2 > 0.0025 = eps_sq)."""
    f = min(d, 8)
    base = 2
    while base ** f < n:
        base += 1
    cell = rng.choice(base ** f, n, replace=False)
    out = rng.uniform(0.1, 0.9, (n, d))
    for i in range(f):
        out[:, i] = 0.1 + spacing * ((cell // base ** i) % base)
    out[:, :f] += rng.uniform(-1e-3, 1e-3, (n, f)) * spacing
    return out


def _shards(blocks):
    """Rank r's points are blocks[r] (equal lengths): the array the group clusters."""
    assert len({len(b) for b in blocks}) == 1
    return np.ascontiguousarray(np.concatenate(blocks))


def relaxed_promotions(seed, d, world=3, per_rank=2500, m_p=100, m_o=2000, minibatch=2500):
    """Promotions the merge makes and no rank made, and the reverse: m_p pcores and m_o outliers on lattice sites 0.6 apart,
    every stored entry k, variances tiny, outlier weights cycling through beta mu - 1, - 2, - 3 (beta mu = 8).  Every rank's shard
    holds one point near outlier j where j % 7 == 0 or j % 14 == 1 (all ranks together lift weights 6 and 5 to beta mu where
    world >= 3, a rank alone only weight 7), rank (j // 7) % world alone one near outlier j where j % 7 == 3, points near the
    pcores, and `far` points near a dozen sites that hold no row (set aside; phase B creates their microclusters).  Outliers j with
    j % 7 == 5 weigh beta mu + 2 and absorb nothing (a stream leaves such rows behind when mu = mu_cfg N falls from one timepoint
    to the next): only rows that absorbed a point in the super-step are promoted.  With
    m_p + m_o = 2 100 rows each of k_rel_promote's 1 024 threads owns three rows, and outliers j, j + 1 share a thread."""
    rng = np.random.default_rng(seed)
    k, beta, mu = 4.0, 0.5, 16.0
    sites = _lattice_sites(rng, m_p + m_o + 12, d)
    cp, co, cfar = sites[:m_p], sites[m_p:m_p + m_o], sites[m_p + m_o:]
    pcores = _table(rng, cp, rng.uniform(0.0, 1e-8, (m_p, d)), k, rng.uniform(10.0, 40.0, m_p))
    j = np.arange(m_o)
    w_o = beta * mu - 1.0 - (j % 3)
    w_o[j % 7 == 5] = beta * mu + 2.0                          # heavy, and no point comes near them: they stay outliers
    outliers = _outlier_table(rng, co, rng.uniform(0.0, 1e-8, (m_o, d)), k, w_o)
    every = j[(j % 7 == 0) | (j % 14 == 1)]
    blocks = []
    for r in range(world):
        own = j[(j % 7 == 3) & ((j // 7) % world == r)]
        near_o = np.concatenate([every, own])
        n_far = min(100, max(0, per_rank - len(near_o)) // 4)
        n_p = per_rank - len(near_o) - n_far
        assert n_p >= 0, "a shard of %d points has no room for %d outlier sites" % (per_rank, len(near_o))
        base = np.concatenate([co[near_o], cp[rng.integers(0, m_p, n_p)], cfar[rng.integers(0, len(cfar), n_far)]])
        blocks.append((base + rng.normal(0.0, 0.002, base.shape))[rng.permutation(per_rank)])
    par = Params(0.05 ** 2, 0.05 ** 2, k, beta, mu, 0.1, 0.5, 0.25, 0.05, d)
    meta = dict(kind="relaxed-promotions", tainted=False, world=world, minibatch=minibatch, full=m_p + m_o > 2048 and world >= 3)
    return pcores, outliers, par, _shards(blocks), meta


def relaxed_divergence(seed, d, world=3, per_rank=100, groups=24, minibatch=64):
    """A promotion a rank makes and the merge refuses, and the reverse.  pi = d - 1, eps 0.1, delta_sq 0.0025, beta mu = 8, outliers of
    weight 7 on lattice sites 0.6 apart, three kinds, `groups` of each:
      X  variance 1.2 delta_sq in dimension 0 (entry 1), tiny elsewhere (entries k): d - 1 entries above 1.  One point on the
         centroid leaves 1.05 delta_sq - the rank promotes, its label carries 4 -, two or three leave 0.93 / 0.84 delta_sq: d
         entries above 1, the merged row stays an outlier;
      Y  variance 0.9 delta_sq in dimension 0 (d entries above 1).  One point at a = sqrt(1.85 delta_sq) beside the centroid in
         dimension 0 leaves 0.990 delta_sq - heavy enough, too many entries -, two or three leave 1.020 / 1.019 delta_sq: d - 1
         entries, the merge promotes by the entry count;
      Z  plain (entries k but one, variance 2 delta_sq there): promoted by every rank that touches it.
    Ranks 0 .. min(world, 3) - 1 hold one point for each X and Y row, every rank one for some Z rows and points near the pcores
    (variance 2 delta_sq in dimension 0, so that the pdim filter lets points join them), a few far from everything."""
    rng = np.random.default_rng(seed)
    assert d >= 2
    k, beta, mu, ds = 4.0, 0.5, 16.0, 0.05 ** 2
    g, m_p = groups, 16
    sites = _lattice_sites(rng, m_p + 3 * g + 4, d)
    cp, co, cfar = sites[:m_p], sites[m_p:m_p + 3 * g], sites[m_p + 3 * g:]
    var_p = rng.uniform(0.0, 1e-8, (m_p, d))
    var_p[:, 0] = 2.0 * ds
    pref_p = np.full((m_p, d), k)
    pref_p[:, 0] = 1.0
    pcores = _table(rng, cp, var_p, pref_p, rng.uniform(10.0, 30.0, m_p))
    perm = rng.permutation(3 * g)
    kind = perm % 3                                          # 0 X, 1 Y, 2 Z, in list order at random
    var = rng.uniform(0.0, 1e-8, (3 * g, d))
    var[:, 0] = np.array([1.2, 0.9, 2.0])[kind] * ds
    pref = np.full((3 * g, d), k)
    pref[kind != 1, 0] = 1.0
    outliers = _outlier_table(rng, co, var, pref, np.full(3 * g, beta * mu - 1.0))
    a = np.sqrt(1.85 * ds)
    x_rows, y_rows, z_rows = (np.flatnonzero(kind == i) for i in range(3))
    sharing = min(world, 3)
    blocks = []
    for r in range(world):
        pts = []
        if r < sharing:
            pts.append(co[x_rows])
            py = co[y_rows].copy()
            py[:, 0] += a
            pts.append(py)
        pts.append(co[z_rows[r % 2::2]])
        n_far = 4
        pts.append(cfar[rng.integers(0, len(cfar), n_far)] + rng.normal(0.0, 1e-3, (n_far, d)))
        have = sum(len(x) for x in pts)
        assert have <= per_rank
        pts.append(cp[rng.integers(0, m_p, per_rank - have)] + rng.normal(0.0, 1e-3, (per_rank - have, d)))
        blocks.append(np.concatenate(pts)[rng.permutation(per_rank)])
    par = Params(0.1 ** 2, ds, k, beta, mu, 0.1, 0.5, 0.25, 0.05, d - 1)
    meta = dict(kind="relaxed-divergence", tainted=False, world=world, minibatch=minibatch, x_uid=outliers.uid[x_rows],
                y_uid=outliers.uid[y_rows])
    return pcores, outliers, par, _shards(blocks), meta


def relaxed_compaction(seed, d, world=3, per_rank=2500, minibatch=2500, first=0):
    """Set-aside points on the pass and wave boundaries of k_rel_collect (1 024 points per pass, 16 waves of 64): 50 pcores and
    20 outliers on lattice sites; rank 0 sets aside its points at `first` + 0, 63, 64, 1 023, 1 024, 2 047, 2 048 and 2 499 (those its
    shard has), rank 1 nothing, rank 2 everything in the first super-step (where `first` is 0), further ranks as rank 0.
    Set-aside points of the first super-step that has any lie near six sites that hold no row: the first of a site creates a
    microcluster in phase B, the others - of whichever rank - join it, and so do rank 2's points of later mini-batches, in
    phase A.  The edge positions of later super-steps have a site each.  Mini-batches start at 2 048 points and double up to the
    configured size: with 2 500, `first` = 2 048 puts the positions into the second super-step, the first of 2 500 points
    (three passes), while at `first` = 0 positions 0 .. 2 047 end the two passes of the first one."""
    rng = np.random.default_rng(seed)
    k, beta, mu = 4.0, 0.5, 16.0
    m_p, m_o, n_new = 50, 20, 6
    edges = np.array([p for p in (0, 63, 64, 1023, 1024, 2047, 2048, 2499) if first + p < per_rank], np.int64) + first
    bounds, pos, size = [], 0, min(minibatch, 2048)
    while pos < per_rank:
        bounds.append(min(per_rank, pos + size))
        pos, size = pos + size, min(minibatch, size * 2)
    step_of = np.searchsorted(np.array(bounds), edges, side="right")
    late = edges[step_of > step_of.min()]
    sites = _lattice_sites(rng, m_p + m_o + n_new + world * len(late), d)
    cp, co, cnew, clate = sites[:m_p], sites[m_p:m_p + m_o], sites[m_p + m_o:m_p + m_o + n_new], sites[m_p + m_o + n_new:]
    pcores = _table(rng, cp, rng.uniform(0.0, 1e-8, (m_p, d)), k, rng.uniform(10.0, 40.0, m_p))
    outliers = _outlier_table(rng, co, rng.uniform(0.0, 1e-8, (m_o, d)), k, rng.uniform(1.0, 3.0, m_o))
    blocks, aside = [], []
    for r in range(world):
        mask = np.zeros(per_rank, bool)
        if r == 2:
            mask[:] = True
        elif r != 1:
            mask[edges] = True
        base = np.where(mask[:, None], cnew[rng.integers(0, n_new, per_rank)],
                        np.concatenate([cp, co])[rng.integers(0, m_p + m_o, per_rank)])
        if r == 2:                                           # (only the first mini-batch's are set aside; see above)
            mask[:] = False
            mask[:bounds[0]] = first == 0
        elif r != 1:
            base[late] = clate[r * len(late):(r + 1) * len(late)]
        blocks.append(base + rng.normal(0.0, 0.002, base.shape))
        aside.append(np.flatnonzero(mask) + r * per_rank)
    par = Params(0.05 ** 2, 0.05 ** 2, k, beta, mu, 0.1, 0.5, 0.25, 0.05, d)
    meta = dict(kind="relaxed-compaction", tainted=False, world=world, minibatch=minibatch, aside=np.concatenate(aside))
    return pcores, outliers, par, _shards(blocks), meta


def relaxed_moving(seed, d, world=2, per_rank=2304, m_p=2048, pairs=64, minibatch=256):
    """Centroids that a merge moves past a neighbouring row: m_p pcores (every entry k, variances tiny), among them `pairs` pairs
    (A, B) with B = A - g e_0, g = 0.02, A of weight 2.  Pair p is served in super-step s = 1 + p % (steps - 2): every rank's
    mini-batch s holds ceil(6 / world) points at A + 1.5 g e_0 (A takes them and ends beyond A + g e_0 in the merge), and
    mini-batch s + 1 of rank p % world holds a probe at A - 0.4 g e_0: A is its nearest row in the table before that merge, B in
    the table after it.  The other points lie near pcores chosen at random.  eps 0.05: every radius test passes."""
    rng = np.random.default_rng(seed)
    k, beta, mu, g = 4.0, 0.5, 16.0, 0.02
    cen = _lattice_sites(rng, m_p, d) if d < 14 else rng.uniform(0.1, 0.9, (m_p, d))
    w = rng.uniform(10.0, 40.0, m_p)
    A, B = np.arange(pairs), pairs + np.arange(pairs)
    cen[B] = cen[A]
    cen[B, 0] -= g
    w[A] = 2.0
    order = rng.permutation(m_p)
    row_of = np.empty(m_p, np.int64)
    row_of[order] = np.arange(m_p)
    pcores = _table(rng, cen[order], rng.uniform(0.0, 1e-8, (m_p, d)), k, w[order])
    steps = []
    pos, size = 0, min(minibatch, 2048)
    while pos < per_rank:
        steps.append((pos, min(per_rank, pos + size)))
        pos, size = pos + size, min(minibatch, size * 2)
    assert len(steps) >= 4
    each = -(-6 // world)
    planned = [[[] for _ in steps] for _ in range(world)]
    e0 = np.zeros(d)
    e0[0] = 1.0
    for p in range(pairs):
        s = 1 + p % (len(steps) - 2)
        for r in range(world):
            planned[r][s] += [cen[A[p]] + 1.5 * g * e0] * each
        planned[p % world][s + 1].append(cen[A[p]] - 0.4 * g * e0)
    blocks = []
    for r in range(world):
        out = []
        for (a, e), special in zip(steps, planned[r]):
            assert len(special) <= e - a
            fill = cen[pairs * 2 + rng.integers(0, m_p - 2 * pairs, e - a - len(special))]
            fill = fill + rng.normal(0.0, 0.002, fill.shape)
            batch = np.concatenate([np.array(special).reshape(-1, d), fill])
            out.append(batch[rng.permutation(e - a)])
        blocks.append(np.concatenate(out))
    par = Params(0.05 ** 2, 0.05 ** 2, k, beta, mu, 0.1, 0.5, 0.25, 0.05, d)
    meta = dict(kind="relaxed-moving", tainted=False, world=world, minibatch=minibatch, A=pcores.uid[row_of[A]],
                B=pcores.uid[row_of[B]])
    return pcores, None, par, _shards(blocks), meta


def relaxed_threshold(seed, d, world=2, per_rank=64, rows=16, minibatch=64):
    """Merged variances exactly ON delta_sq.  delta_sq = 1/16, eps 1/2; `rows` pcores and as many outliers of weight 2 whose
    centroid is 8 + 2 i in dimension 0 (far from every other row, which lie on lattice sites below 4) with variance 1/16 there.
    Rank 0 holds a point 1/4 above each such centroid, rank 1 one 1/4 below: alone either leaves 1/16 - 1/144, together W = 4,
    CF1 / W the old centroid and CF2 / W - (CF1 / W)^2 = 1/16 - every term a small dyadic number, every sum exact -, so the merged
    entry is k by `<=` and would be 1 by `<`.  Further ranks and the other points: near plain pcores."""
    rng = np.random.default_rng(seed)
    assert world >= 2 and d >= 2
    k, beta, mu = 4.0, 0.5, 16.0
    m_plain = 8
    sites = _lattice_sites(rng, m_plain + 2 * rows, d)
    cen = sites.copy()
    cen[m_plain:, 0] = 8.0 + 2.0 * np.arange(2 * rows)
    var = rng.uniform(0.0, 1e-8, (m_plain + 2 * rows, d))
    var[m_plain:, 0] = 1.0 / 16.0
    w = np.concatenate([rng.uniform(10.0, 40.0, m_plain), np.full(2 * rows, 2.0)])
    on_p = np.arange(m_plain + rows)
    on_o = m_plain + rows + np.arange(rows)
    pcores = _table(rng, cen[on_p], var[on_p], k, w[on_p])
    outliers = _outlier_table(rng, cen[on_o], var[on_o], k, w[on_o])
    blocks = []
    for r in range(world):
        pts = []
        if r < 2:
            x = cen[m_plain:].copy()
            x[:, 0] += 0.25 if r == 0 else -0.25
            pts.append(x)
        have = sum(len(x) for x in pts)
        assert have <= per_rank
        pts.append(cen[rng.integers(0, m_plain, per_rank - have)] + rng.normal(0.0, 1e-3, (per_rank - have, d)))
        blocks.append(np.concatenate(pts)[rng.permutation(per_rank)])
    par = Params(0.25, 1.0 / 16.0, k, beta, mu, 0.1, 0.5, 0.25, 0.05, d)
    meta = dict(kind="relaxed-threshold", tainted=False, world=world, minibatch=minibatch,
                uids=np.concatenate([pcores.uid[m_plain:], outliers.uid]))
    return pcores, outliers, par, _shards(blocks), meta


def relaxed_tainted(seed, d, world=2, minibatch=64, m_p=60, m_o=60, n=300, **kw):
    """`stale` as the relaxed mode sees it: stored entries that disagree with the variances (the handle is tainted).  A row that
    absorbs a point on any rank gets entries of k and 1 in the merge; a row that absorbs none keeps its stored ones."""
    pcores, outliers, par, X, meta = stale(seed, m_p, m_o, d, n, **kw)
    meta = dict(meta, kind="relaxed-tainted", world=world, minibatch=minibatch)
    return pcores, outliers, par, X, meta


def relaxed_victims(seed, d, world=3, minibatch=64, pairs=40, **kw):
    pcores, outliers, par, X, meta = victims(seed, pairs, d, points=pairs // 2, **kw)
    meta = dict(meta, kind="relaxed-tainted", world=world, minibatch=minibatch)
    return pcores, outliers, par, X, meta


def model_relaxed(case, world=None, minibatch=None):
    """The model's side of a relaxed case (relaxed_model.relaxed_online on the injected tables); world / minibatch other than
    the case's own run the same points in another group (the structure conditions then need not hold)."""
    import relaxed_model as R
    pcores, outliers, par, X, meta = case
    state = R.state_of(make_oracle(par, pcores, outliers), X.shape[1])
    return R.relaxed_online(par, state, X, world or meta["world"], minibatch or meta["minibatch"])


def _nearest(X, t):
    """Per point the uid of the nearest row of table t (projected distance, first minimum)."""
    out = np.empty(len(X), np.int64)
    for a in range(0, len(X), 64):
        x = X[a:a + 64]
        dist = ((x[:, None, :] - t["cen"][None, :, :]) ** 2 / t["pref"][None, :, :]).sum(axis=2)
        out[a:a + 64] = t["uid"][dist.argmin(axis=1)]
    return out


def check_relaxed(case, res):
    """Asserts on the MODEL's result that the case holds what it exists for (no GPU involved); returns the counts behind the
    conditions."""
    pcores, outliers, par, X, meta = case
    kind, steps = meta["kind"], res["steps"]
    counts = {}
    local_up = [set() for _ in steps]                         # uids some rank promoted in phase A, per super-step
    for s, st in enumerate(steps):
        for lu, lp in st["local"]:
            local_up[s] |= set(int(u) for u in lu[(lp >= 0) & (lp & 4 != 0) & (lp != 8)])
    if kind == "relaxed-promotions":
        info = steps[0]["info"]
        m = len(info["w"])
        per = -(-m // 1024)
        rows = info["promoted"]
        uids = [int(u) for u in info["rows"]["uid"][rows]]
        merged_only = [u for u in uids if u not in local_up[0]]
        threads = rows // per
        idle_heavy = (~info["touched"]) & info["heavy"] & ((info["pref"] > 1.0).sum(axis=1) <= par.pi)
        idle_heavy[:info["n_pcore"]] = False
        kept = set(int(u) for u in res["state"]["outlier"]["uid"])
        assert idle_heavy.sum() >= 8 and all(int(u) in kept for u in info["rows"]["uid"][idle_heavy]), int(idle_heavy.sum())
        counts = dict(rows=m, rows_per_thread=per, promotions=len(rows), merged_only=len(merged_only),
                      heavy_outliers_left_alone=int(idle_heavy.sum()),
                      also_local=len(uids) - len(merged_only), threads=len(np.unique(threads)),
                      pairs_in_a_thread=int((np.diff(threads) == 0).sum()), set_aside=res["stats"]["deferred_points"])
        if meta["full"]:
            assert per >= 3, counts
            assert counts["merged_only"] >= 32 and counts["also_local"] >= 32, counts
            assert counts["pairs_in_a_thread"] >= 1 and counts["threads"] >= 8, counts
    elif kind == "relaxed-divergence":
        outl = set(int(u) for u in res["state"]["outlier"]["uid"])
        pc = set(int(u) for u in res["state"]["pcore"]["uid"])
        all_local = set().union(*local_up)
        refused = [int(u) for u in meta["x_uid"] if int(u) in all_local and int(u) in outl]
        by_count = []
        for s, st in enumerate(steps):
            if st["info"] is None:
                continue
            info = st["info"]
            beta_mu = par.beta * par.mu
            heavy_somewhere = np.zeros(len(info["w"]), bool)
            for dw in info["dw_by_rank"]:
                heavy_somewhere |= (dw != 0.0) & (info["rows"]["w"] + dw >= beta_mu)
            for r in info["promoted"]:
                u = int(info["rows"]["uid"][r])
                if u not in local_up[s] and heavy_somewhere[r]:
                    by_count.append(u)
        counts = dict(local_promotion_refused=len(refused), merged_by_entry_count=len(by_count),
                      of_them_y=len(set(by_count) & set(int(u) for u in meta["y_uid"])))
        if meta["world"] >= 2:
            assert len(refused) >= 1 and len(by_count) >= 1 and set(by_count) <= pc, counts
    elif kind == "relaxed-compaction":
        aside = np.flatnonzero(np.isin(np.arange(len(X)), np.concatenate([st["deferred"] for st in steps])))
        assert np.array_equal(aside, meta["aside"]), "the set-aside points are not the planned ones"
        shard = -(-len(X) // meta["world"])
        joined_other = set()
        for st in steps:
            bu, bp = st["b"]
            created = {}
            for i, u, p in zip(st["deferred"], bu, bp):
                if p == 2:
                    created[int(u)] = int(i) // shard
                elif int(u) in created and created[int(u)] != int(i) // shard:
                    joined_other.add(int(u))
        counts = dict(set_aside=res["stats"]["deferred_points"], by_step=[len(st["deferred"]) for st in steps],
                      created_and_joined_by_other_ranks=len(joined_other))
        assert counts["set_aside"] == len(meta["aside"])
        if meta["world"] >= 3:
            assert len(joined_other) >= 2, counts
    elif kind == "relaxed-moving":
        changed, a_to_b = 0, 0
        pair = dict(zip((int(u) for u in meta["A"]), (int(u) for u in meta["B"])))
        for s in range(1, len(steps)):
            before, after = steps[s - 1]["before"]["pcore"], steps[s]["before"]["pcore"]
            for a, e in steps[s]["ranges"]:
                nb, na = _nearest(X[a:e], before), _nearest(X[a:e], after)
                changed += int((nb != na).sum())
                a_to_b += sum(1 for x, y in zip(nb, na) if pair.get(int(x)) == int(y))
        counts = dict(merges=len(steps), nearest_row_changed_by_a_merge=changed, from_A_to_B=a_to_b)
        assert len(steps) >= 8 and changed >= 16, counts
    elif kind == "relaxed-threshold":
        on = 0
        want = set(int(u) for u in meta["uids"])
        for st in steps:
            for name in ("pcore", "outlier"):
                t = st["merged"][name]
                sel = np.array([int(u) in want for u in t["uid"]], bool)
                var = t["cf2"][sel, 0] / t["w"][sel] - (t["cf1"][sel, 0] / t["w"][sel]) ** 2
                hit = (var == par.delta_sq) & (t["w"][sel] == 4.0)
                assert (t["pref"][sel, 0][hit] == par.k).all()
                on += int(hit.sum())
        counts = dict(merged_variances_on_delta_sq=on, rows=len(want))
        assert on == len(want), counts
    elif kind == "relaxed-tainted":
        touched = {}
        for st in steps:
            if st["info"] is not None:
                for u, t in zip(st["info"]["rows"]["uid"], st["info"]["touched"]):
                    touched[int(u)] = touched.get(int(u), False) or bool(t)
            for u in st["b"][0]:
                touched[int(u)] = True
        final = {int(u): res["state"][name]["pref"][r] for name in ("pcore", "outlier")
                 for r, u in enumerate(res["state"][name]["uid"])}
        for name, t in (("pcores", pcores), ("outliers", outliers)):
            if t is None:
                continue
            hit = np.array([touched.get(int(u), False) for u in t.uid])
            counts[name] = dict(touched=int(hit.sum()), untouched=int((~hit).sum()))
            for r in np.flatnonzero(~hit):
                assert np.array_equal(final[int(t.uid[r])].view(np.int64), t.pref[r].view(np.int64)), "an untouched row's entries changed"
            if meta.get("full", True) or len(t) >= 31:
                assert hit.any() and not hit.all(), (name, counts)
    else:
        raise ValueError(kind)
    return counts


# every case of tests/test_relaxed_model.py and tests/test_relaxed_model_cpu.py: name -> (generator, arguments).  At most 2 148
# rows and 7 500 points.  Widths: 3 below the ladder, 8, 13 and 37 over padded operands, 20 and 40 on the ladder, 64 the last
# windowed one.
RELAXED_DIMS = (3, 8, 13, 20, 37, 40, 64)
RELAXED_TABLES = {}
for _d in RELAXED_DIMS:
    RELAXED_TABLES["divergence-3x100x%d" % _d] = (relaxed_divergence, dict(seed=400 + _d, d=_d))
    RELAXED_TABLES["tainted-2x150x%d" % _d] = (relaxed_tainted, dict(seed=500 + _d, d=_d))
    RELAXED_TABLES["victims-3x20x%d" % _d] = (relaxed_victims, dict(seed=600 + _d, d=_d))
    RELAXED_TABLES["promotions-small-3x200x%d" % _d] = (relaxed_promotions, dict(seed=700 + _d, d=_d, per_rank=200, m_p=20, m_o=210,
                                                                            minibatch=256))
    RELAXED_TABLES["threshold-2x64x%d" % _d] = (relaxed_threshold, dict(seed=750 + _d, d=_d))
for _d in (8, 20):
    RELAXED_TABLES["promotions-3x2500x%d" % _d] = (relaxed_promotions, dict(seed=800 + _d, d=_d))
for _d in (8, 13, 37):
    RELAXED_TABLES["compaction-3x2500x%d" % _d] = (relaxed_compaction, dict(seed=900 + _d, d=_d))
RELAXED_TABLES["compaction-1x5000x8"] = (relaxed_compaction, dict(seed=950, d=8, world=1, per_rank=5000, first=2048))
RELAXED_TABLES["compaction-4x1875x20"] = (relaxed_compaction, dict(seed=951, d=20, world=4, per_rank=1875))
for _d in (20, 40):
    RELAXED_TABLES["moving-2x2304x%d" % _d] = (relaxed_moving, dict(seed=1000 + _d, d=_d))
    RELAXED_TABLES["tainted-3x700x%d" % _d] = (relaxed_tainted, dict(seed=1100 + _d, d=_d, world=3, minibatch=256, m_p=1400,
                                                                    m_o=700, n=2100, filt=_d == 20))
del _d


# the stream of the decay tests: timepoints 0, 1 and 3 with lambda = 0.5 (factors 2^-0.5 and 2^-1: fractional weights), 15 % of
# the blobs replaced per timepoint, promotion after 40 points and omicron 3 points: retired blobs are downgraded, light outlier
# microclusters deleted (tests/test_relaxed_model_cpu.py counts them)
RELAXED_DECAY = dict(seed=31, n=3000, d=14, g=40, sigma=0.01, timepoints=3, drift=0.005, churn=0.15)
RELAXED_DECAY_DAYS = [0, 1, 3]


def relaxed_decay_config():
    import scenarios
    return scenarios.params_to_config(scenarios.blob_params(RELAXED_DECAY["n"], promote_after=40, param_lambda=0.5,
                                                            param_omicron=0.001))


def build_relaxed(name):
    gen, kw = RELAXED_TABLES[name]
    return gen(**kw)


if __name__ == "__main__":  # the structure conditions of every table against the oracle alone (no GPU)
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    unknown = [a for a in sys.argv[1:] if a not in ONLINE_TABLES and a not in OFFLINE_TABLES]
    if unknown:
        sys.exit("no such table: %s" % ", ".join(unknown))
    for name in [a for a in sys.argv[1:] if a in ONLINE_TABLES] or ([] if sys.argv[1:] else ONLINE_TABLES):
        t0 = time.time()
        case = build_online(name)
        t1 = time.time()
        res = oracle_online(case)
        check_online(case, res)
        print("%-30s ok: %5d + %5d rows, %4d points, paths %s, build %.1f s, oracle %.1f s" % (
            name, len(case[0]) if case[0] is not None else 0, len(case[1]) if case[1] is not None else 0, len(case[3]),
            dict(zip(*[x.tolist() for x in np.unique(res["path"], return_counts=True)])), t1 - t0, time.time() - t1))
    for name in [a for a in sys.argv[1:] if a in OFFLINE_TABLES] or ([] if sys.argv[1:] else OFFLINE_TABLES):
        t0 = time.time()
        t, par, meta = build_table(name)
        info, clusters = oracle_offline(make_oracle(par, t))
        check_structure(t, par, meta, info, clusters)
        print("%-26s ok: %5d pcores, %5d core, %5d clusters (largest %d), nn %d..%d, nw %d..%d, %.1f s" % (
            name, len(t), info["num_core"], len(clusters), max([len(c["members"]) for c in clusters] or [0]),
            info["nn"].min(), info["nn"].max(), info["nw"].min(), info["nw"].max(), time.time() - t0))
