"""Designed ARRIVALS for the validation rounds of the online phase (csrc/cc_validate.h: k_dseed, k_decide, k_chain, k_chain_long,
k_claims, k_claims_heavy, k_commit_a / b, the carry set): what happens INSIDE a window.

The blob streams of the parity suites arrive in i.i.d. order and meet a chain length only by chance.  Here the geometry is
trivial - sites far apart, one tight injected microcluster per site, every point within a small offset of its site, so that
its nearest row is its site's by a wide margin - and the schedule is the design: the row sequence lab[0 .. n) is periodic with
period W, the configured window, so every run of W consecutive points holds exactly L_i points of row i wherever a window
begins.  Lengths sit on the packed limits of the kernels (the member list of 32, k_chain_long's batch K(d), its queue of
2 048), members arrive `robin` (exactly W / L apart), in a `burst`, `head+tail` (the list holds the earliest members, a lookup
from the tail is out of reach of k_dseed's walk and of its backward read), the whole call `sorted` by row, or `shuffled` (the
i.i.d. twin with the same multiset of points).  Events land on chosen chain steps:

  breathing rows   members alternate c +- a e_0 with a^2 = 2.125 delta^2 and delta^2 / k < eps^2 < delta^2: the variance of dimension
                   0 crosses delta^2 at a step fixed by the row's weight, the entry flips from k to 1 and the radius test fails
                   from that step on (every member passes against the snapshot row: all of them claim it, the chain rejects);
  promotions       an outlier row of weight beta mu - s - 1 is promoted by its member s; a light pcore row 3.5 delta beside it
                   rejects the members (tentative variance above delta^2) and absorbs the flip points 1.3 delta on its side of
                   the promoted row - until the promotion, after which they are nearer to the promoted row;
  creations        a site with no row: one creator, L followers through the promotion of the new row.

`arrivals` returns the 5-tuple of table_util.build_online, so oracle_online / handle_online / same_online / group_online serve
it unchanged; `check_arrivals` asserts on the ORACLE's result alone that the design holds."""
import numpy as np

import table_util as T
from table_util import Params

EPS, DELTA = 0.006, 0.008        # delta^2 / 4 < eps^2 < delta^2 (k = 4): a dimension that flips to 1 fails the radius test
SIGMA = 2e-4                     # spread of plain members around their site
SEP = 10.0 * EPS                 # sites at least this far apart
SHIELD = 3.5 * DELTA             # a light pcore row this far from an outlier / empty site rejects the site's points
FLIP = 1.3 * DELTA               # flip points: this far from the promoted row, SHIELD - FLIP from the shield
N_FILLER = 1100


def chain_batch(d):
    """Steps per batch of k_chain_long (cc_validate.h; tests/test_arrival_orders_cpu.py holds it against the source line)."""
    return min(256, (6144 // (2 * d)) & ~7)


def _place(rng, seps, d, lo=0.1, hi=0.9):
    """len(seps) sites of [lo, hi)^d, site i at least max(seps[i], seps[j]) from site j; the demanding ones are drawn first."""
    order = np.argsort(-np.asarray(seps), kind="stable")
    out = np.empty((len(seps), d))
    done, tries = [], 0
    for i in order:
        while True:
            c = rng.uniform(lo, hi, d)
            tries += 1
            assert tries < 400 * len(seps) + 4000, "no room for %d sites in %d dimensions" % (len(seps), d)
            if all(((out[j] - c) ** 2).sum() >= max(seps[i], seps[j]) ** 2 for j in done):
                break
        out[i] = c
        done.append(i)
    return out


def _first_rejected(c0, v0, w0, a, s_max, delta_sq):
    """The member (0-based) of a breathing row of weight w0 at which dimension 0's tentative variance first exceeds delta_sq,
    in the oracle's own expressions (cf2 / w - (cf1 / w)^2); members alternate c0 + a, c0 - a."""
    cf1, cf2, w = c0 * w0, (v0 + c0 * c0) * w0, w0
    for m in range(s_max + 1):
        x = c0 + a if m % 2 == 0 else c0 - a
        w1 = w + 1.0
        b = (cf1 + x) / w1
        if (cf2 + x * x) / w1 - b * b > delta_sq:
            return m
        cf1, cf2, w = cf1 + x, cf2 + x * x, w1
    return None


def _schedule(W, specs):
    """owner[0 .. W): the row (index into specs) of every point of one period.  Bursts and head / tail members take their
    slots first, robin rows (longest first) theirs or the next free one, `fill` rows share what is left in turn."""
    owner = np.full(W, -1, np.int64)

    def put(i, positions, strict=False):
        for p in positions:
            p = int(p) % W
            assert not strict or owner[p] == -1, "slot %d is taken" % p
            while owner[p] != -1:
                p = (p + 1) % W
            owner[p] = i

    def put_tail(i, count):
        p = W - 1
        for _ in range(count):
            while owner[p] != -1:
                p -= 1
            owner[p] = i

    for i, sp in enumerate(specs):
        pat = sp["pat"]
        if pat[0] == "burst":
            put(i, pat[1] + np.arange(sp["L"]), strict=True)
    for i, sp in enumerate(specs):
        pat = sp["pat"]
        if pat[0] == "headtail":
            mid = pat[1]
            assert sp["L"] > 32 + mid
            put(i, 2 * np.arange(32))                       # 32 members in the first 64 points
            put(i, W // 2 + np.arange(mid), strict=True)
            put_tail(i, sp["L"] - 32 - mid)
            assert (np.flatnonzero(owner == i)[-(sp["L"] - 32 - mid):] >= W - 64).all()
    robin = [i for i, sp in enumerate(specs) if sp["pat"][0] == "robin"]
    for i in sorted(robin, key=lambda r: -specs[r]["L"]):
        L = specs[i]["L"]
        put(i, specs[i]["pat"][1] + (np.arange(L) * W) // L)
    fill = [i for i, sp in enumerate(specs) if sp["pat"][0] == "fill"]
    free = np.flatnonzero(owner == -1)
    assert len(fill) or len(free) == 0, "%d slots of the period have no row" % len(free)
    for n, p in enumerate(free):
        owner[p] = fill[n % len(fill)]
    for i, sp in enumerate(specs):
        if sp["pat"][0] == "fill":
            sp["L"] = int((owner == i).sum())
        assert int((owner == i).sum()) == sp["L"], (i, sp)
    return owner


def plain(L, pat=("robin", 0)):
    return dict(kind="plain", L=L, pat=pat)


def breath(s, L, pat=("robin", 0), centre=False):
    return dict(kind="breath", L=L, pat=pat, s=s, centre=centre)


def promo(s, L, pat=("robin", 0)):
    return dict(kind="promo", L=L, pat=pat, s=s)


def create(L, pat=("robin", 0)):
    return dict(kind="create", L=L, pat=pat)


def arrivals(seed, d, W, specs, order="period", large=False, filt=False, k=4.0, beta_mu=1e9, periods=3):
    """specs: rows as built by plain / breath / promo / create (L members per period, pattern pat); order: `period` (the
    designed schedule, `periods` times), `sorted` (the whole call sorted by row) or `shuffled` (a random permutation of it).
    large: about 1 100 filler rows in a far corner beside the active ones.  filt: pi = d - 1, every row carries the variance
    2 delta^2 in its last dimension and its members keep it there (eps^2 = 4 delta^2; plain rows only)."""
    rng = np.random.default_rng(seed)
    specs = [dict(sp) for sp in specs]
    delta_sq = DELTA * DELTA
    eps_sq = 4.0 * delta_sq if filt else EPS * EPS
    assert filt or delta_sq / k < eps_sq < delta_sq
    assert not filt or all(sp["kind"] == "plain" for sp in specs)
    a = np.sqrt(2.125) * DELTA                               # (not 2: a variance ON delta^2 would be decided by rounding)
    n_rows = len(specs)
    # a breathing row leaves two outlier rows of up to periods L / 2 points behind, which absorb what comes within 2 eps sqrt(w)
    seps = [max(SEP, 2.5 * EPS * np.sqrt(0.5 * periods * sp["L"] + 8.0)) if sp["kind"] == "breath" else
            (max(SEP, 2.0 * SHIELD + SEP) if sp["kind"] in ("promo", "create") else SEP) for sp in specs]
    sites = _place(rng, seps, d)
    e0 = np.zeros(d)
    e0[0] = 1.0

    owner = _schedule(W, specs)
    lab = np.tile(owner, periods)
    n = len(lab)
    if order == "sorted":
        rank = rng.permutation(n_rows)
        lab = lab[np.argsort(rank[lab], kind="stable")]
    elif order == "shuffled":
        lab = lab[rng.permutation(n)]
    else:
        assert order == "period"
    by_row = np.argsort(lab, kind="stable")                  # the points of row 0 in arrival order, then row 1's, ...
    starts = np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=n_rows))])

    # the table: one pcore row per plain / breathing site, an outlier row per promotion site, a light pcore row (the shield)
    # beside every promotion and creation site, the fillers
    p_cen, p_w, p_site, o_cen, o_w, o_site = [], [], [], [], [], []
    for i, sp in enumerate(specs):
        if sp["kind"] == "plain":
            p_cen.append(sites[i]); p_w.append(10.0); p_site.append(i)
        elif sp["kind"] == "breath":
            p_cen.append(sites[i]); p_w.append(0.0); p_site.append(i)       # (weight set below)
        elif sp["kind"] == "promo":
            assert beta_mu - sp["s"] - 1.0 >= 1.0
            o_cen.append(sites[i]); o_w.append(beta_mu - sp["s"] - 1.0); o_site.append(i)
        if sp["kind"] in ("promo", "create"):
            p_cen.append(sites[i] - SHIELD * e0); p_w.append(6.0 if sp["kind"] == "promo" else 4.0); p_site.append(-1 - i)
    n_act_p, n_act_o = len(p_cen), len(o_cen)
    if large:
        n_fo = 100
        p_cen += list(rng.uniform(3.0, 4.0, (N_FILLER - n_fo, d))); p_w += [10.0] * (N_FILLER - n_fo)
        p_site += [None] * (N_FILLER - n_fo)
        o_cen += list(rng.uniform(-4.0, -3.0, (n_fo, d))); o_w += [2.0] * n_fo; o_site += [None] * n_fo
    p_cen, p_w = np.array(p_cen).reshape(-1, d), np.array(p_w)
    p_var = rng.uniform(0.0, 1e-10, p_cen.shape)
    if filt:
        p_var[:, d - 1] = 2.0 * delta_sq
    for r in range(n_act_p):                                 # the weight of a breathing row: the one that rejects member s first
        sp = specs[p_site[r]] if p_site[r] is not None and p_site[r] >= 0 else None
        if sp is not None and sp["kind"] == "breath":
            w0 = next((w for w in range(1, 2 * sp["s"] + 16)
                       if _first_rejected(p_cen[r, 0], p_var[r, 0], float(w), a, sp["s"] + 2, delta_sq) == sp["s"]), None)
            assert w0 is not None, "no integer weight rejects member %d first" % sp["s"]
            p_w[r] = float(w0)
    p_pref = np.where(p_var <= delta_sq, k, 1.0)
    perm = rng.permutation(len(p_w))
    pcores = T._table(rng, p_cen[perm], p_var[perm], p_pref[perm], p_w[perm])
    p_uid = np.empty(len(p_w), np.int64)
    p_uid[perm] = pcores.uid
    outliers = None
    o_uid = np.zeros(0, np.int64)
    if len(o_w):
        o_cen = np.array(o_cen).reshape(-1, d)
        perm_o = rng.permutation(len(o_w))
        outliers = T._outlier_table(rng, o_cen[perm_o], rng.uniform(0.0, 1e-10, o_cen.shape), k, np.array(o_w)[perm_o])
        o_uid = np.empty(len(o_w), np.int64)
        o_uid[perm_o] = outliers.uid
    row_uid = np.full(n_rows, -1, np.int64)                  # the uid of the site's own row (-1: the call creates it)
    shield_uid = np.full(n_rows, -1, np.int64)
    for r in range(n_act_p):
        if p_site[r] >= 0:
            row_uid[p_site[r]] = p_uid[r]
        else:
            shield_uid[-1 - p_site[r]] = p_uid[r]
    for r in range(n_act_o):
        row_uid[o_site[r]] = o_uid[r]

    # the points, row by row in arrival order, and what the design says of each
    X = np.empty((n, d))
    want_uid = np.full(n, -1, np.int64)                      # -1: not fixed by the design
    want_path = np.full(n, -1, np.int64)
    events = []
    for i, sp in enumerate(specs):
        idx = by_row[starts[i]:starts[i + 1]]
        m = len(idx)
        c = sites[i]
        if sp["kind"] == "plain":
            pts = c + rng.normal(0.0, SIGMA, (m, d))
            if filt:
                pts[:, d - 1] = c[d - 1] + a * np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
            want_uid[idx], want_path[idx] = row_uid[i], 0
        elif sp["kind"] == "breath":
            s = sp["s"]
            assert m > s + 1
            pts = np.tile(c, (m, 1))
            o = np.arange(m)
            is_centre = (o > s) & ((o - s) % 3 == 1) if sp["centre"] else np.zeros(m, bool)
            swing = np.cumsum(~is_centre) - 1                # ordinal among the swinging members
            pts[:, 0] += np.where(is_centre, 0.0, np.where(swing % 2 == 0, a, -a))
            want_uid[idx[:s]], want_path[idx[:s]] = row_uid[i], 0
            events.append(dict(kind="breath", row=i, members=idx, s=s, centre=sp["centre"]))
        elif sp["kind"] == "promo":
            s = sp["s"]
            assert m > s + 4
            pts = c + rng.normal(0.0, 1e-5, (m, d))
            flips = np.array([0, s + 2, s + 3])               # [flip, m_0 .. m_s, flip, flip, m_s+1 ...]
            pts[flips] = c - FLIP * e0
            member = np.ones(m, bool)
            member[flips] = False
            mem = idx[member]
            want_uid[idx], want_path[idx] = row_uid[i], 0
            want_path[mem[:s]] = 1
            want_path[mem[s]] = 5
            want_uid[idx[0]] = shield_uid[i]
            events.append(dict(kind="promo", row=i, members=mem, s=s, flips=idx[flips], shield=int(shield_uid[i])))
        elif sp["kind"] == "create":
            pts = c + rng.normal(0.0, 1e-5, (m, d))
            events.append(dict(kind="create", row=i, members=idx))
        X[idx] = pts

    par = Params(eps_sq, delta_sq, k, 0.5, 2.0 * beta_mu, 0.1, 0.5, 0.25, 0.05, d - 1 if filt else d)
    meta = dict(kind="arrivals", tainted=False, W=W, periods=periods, order=order, large=large, lab=lab, specs=specs,
                L=np.array([sp["L"] for sp in specs]), row_uid=row_uid, want_uid=want_uid, want_path=want_path, events=events,
                breathing=any(sp["kind"] == "breath" for sp in specs), longest=max(sp["L"] for sp in specs))
    return pcores, outliers, par, np.ascontiguousarray(X), meta


def check_arrivals(case, res):
    """Asserts on the ORACLE's result that the case holds its design (no GPU involved)."""
    pcores, outliers, par, X, meta = case
    uid, path = res["uid"], res["path"]
    W, lab, L = meta["W"], meta["lab"], meta["L"]
    if meta["order"] == "period":                            # every run of W points holds exactly L_i points of row i
        for p in range(meta["periods"]):
            assert np.array_equal(np.bincount(lab[p * W:(p + 1) * W], minlength=len(L)), L), "period %d" % p
        assert np.array_equal(lab[W:], lab[:-W])
    assert np.array_equal(np.bincount(lab, minlength=len(L)), meta["periods"] * L)
    fixed = meta["want_uid"] >= 0
    bad = np.flatnonzero(fixed & (uid != meta["want_uid"]))
    assert len(bad) == 0, "%d points not absorbed by the row the design names, the first at %d (row %d)" % (
        len(bad), bad[0], lab[bad[0]])
    fixed = meta["want_path"] >= 0
    bad = np.flatnonzero(fixed & (path != meta["want_path"]))
    assert len(bad) == 0, "%d points off the designed path, the first at %d (row %d): %d for %d" % (
        len(bad), bad[0], lab[bad[0]], path[bad[0]], meta["want_path"][bad[0]])
    for i, sp in enumerate(meta["specs"]):                   # per period, each plain row's count is L_i
        if sp["kind"] == "plain" and meta["order"] == "period":
            for p in range(meta["periods"]):
                assert int((uid[p * W:(p + 1) * W] == meta["row_uid"][i]).sum()) == sp["L"]
    for ev in meta["events"]:
        mem = ev["members"]
        if ev["kind"] == "breath":
            s, own = ev["s"], meta["row_uid"][ev["row"]]
            assert (path[mem[:s]] == 0).all() and (uid[mem[:s]] == own).all()
            assert path[mem[s]] in (1, 2) and uid[mem[s]] != own, "member %d of row %d was not rejected" % (s, ev["row"])
            if ev["centre"]:                                  # centre points bring the variance back: a later step is accepted
                assert (uid[mem[s + 1:]] == own).any() and (uid[mem[s + 1:]] != own).any()
        elif ev["kind"] == "promo":
            s, own = ev["s"], meta["row_uid"][ev["row"]]
            assert (path[mem[:s]] == 1).all() and path[mem[s]] == 5 and (path[mem[s + 1:]] == 0).all()
            assert (uid[mem] == own).all()
            f = ev["flips"]
            assert uid[f[0]] == ev["shield"] and (uid[f[1:]] == own).all() and (path[f] == 0).all()
            assert f[0] < mem[s] < f[1], "the flip points do not straddle the promotion"
        elif ev["kind"] == "create":
            assert path[mem[0]] == 2 and int((path[mem] == 2).sum()) == 1, "row %d: %d creations" % (
                ev["row"], int((path[mem] == 2).sum()))
            assert (uid[mem] == uid[mem[0]]).all()
            if len(mem) > par.beta * par.mu:
                assert int((path[mem] == 5).sum()) == 1


# ---- the cases ------------------------------------------------------------------------------------------------------------
# name -> arguments of `arrivals`.  W = 4 096 and n = 12 288 unless the name says otherwise; `-large`: beside 1 100 fillers.

def _lens(d, W=4096):
    """Every designed length that fits one period beside the others: 1, the list's 31 .. 34, K - 1 .. K + 1, 2 K, 2 K + 1 and
    2 047 (the queue of 2 048, less one), robin; three rows share the rest."""
    K = chain_batch(d)
    rows = [plain(L, ("robin", 7 * j)) for j, L in enumerate([1, 31, 32, 33, 34, K - 1, K, K + 1, 2 * K, 2 * K + 1, 2047])]
    return rows + [plain(0, ("fill",)) for _ in range(3)]


def _bursts(d, W=4096):
    """Bursts at the start of the period, ending on its last point, across a 64-point tile edge and across a 16-row version
    tile; two robin rows and the fill between them."""
    K = chain_batch(d)
    return [plain(33, ("burst", 0)), plain(K + 1, ("burst", W - (K + 1))), plain(34, ("burst", 1024 - 17)),
            plain(2 * K + 1, ("burst", 2048 + 16 - 5)), plain(K, ("burst", 3000)), plain(32, ("burst", 600)),
            plain(K - 1, ("robin", 3)), plain(257, ("robin", 11))] + [plain(0, ("fill",)) for _ in range(3)]


def _headtail(d, W=4096):
    """head+tail: 32 members in the first 64 points, the rest in the last 64; the second row with 70 members in the middle of
    the period as well - from its tail the listed members are 70 chain steps and half a window away."""
    return [plain(32 + 44, ("headtail", 0)), plain(32 + 70 + 20, ("headtail", 70)), plain(33, ("robin", 5)),
            plain(2047, ("robin", 9))] + [plain(0, ("fill",)) for _ in range(3)]


def _breathing(d, large=False):
    K = chain_batch(d)
    L = 2 * K + 1
    steps = [1, 32, 33, K - 1, K, K + 1]
    rows = [breath(s, L, ("robin", 5 * j)) for j, s in enumerate(steps)]
    rows.append(breath(K, L, ("robin", 31), centre=True))    # accepted steps behind the first rejected one: replays resume
    rows.append(breath(33, 34, ("robin", 41), centre=True))
    return rows + [plain(0, ("fill",)) for _ in range(2)]


def _promotions(d):
    K = chain_batch(d)
    L = 2 * K + 5
    return [promo(s, L, ("robin", 5 * j)) for j, s in enumerate([1, 32, 33, K - 1, K, K + 1])] + \
        [plain(0, ("fill",)) for _ in range(3)]


def _creations(d):
    return [create(L + 1, ("robin", 5 * j)) for j, L in enumerate([1, 33, 34, 257, 2047])] + \
        [plain(33, ("robin", 3)), plain(0, ("fill",)), plain(0, ("fill",))]


def _many(d, rows=297):
    """A table of 300 rows: every row a chain of 13 or 14, three long ones."""
    return [plain(33, ("robin", 1)), plain(34, ("robin", 2)), plain(257, ("robin", 3))] + [plain(0, ("fill",)) for _ in range(rows)]


ARRIVAL_CASES = {}
for _d in (3, 6, 14, 20, 40, 64):
    ARRIVAL_CASES["lens-robin-d%d" % _d] = dict(seed=1000 + _d, d=_d, W=4096, specs=_lens(_d))
    ARRIVAL_CASES["breath-robin-d%d" % _d] = dict(seed=1100 + _d, d=_d, W=4096, specs=_breathing(_d))
for _d in (6, 20):
    for _o in ("sorted", "shuffled"):
        ARRIVAL_CASES["lens-%s-d%d" % (_o, _d)] = dict(seed=1000 + _d, d=_d, W=4096, specs=_lens(_d), order=_o)
        ARRIVAL_CASES["breath-%s-d%d" % (_o, _d)] = dict(seed=1100 + _d, d=_d, W=4096, specs=_breathing(_d), order=_o)
    for _o in ("period", "sorted", "shuffled"):
        _n = "robin" if _o == "period" else _o
        ARRIVAL_CASES["lens-%s-d%d-large" % (_n, _d)] = dict(seed=1200 + _d, d=_d, W=4096, specs=_lens(_d), order=_o, large=True)
        ARRIVAL_CASES["promo-%s-d%d" % (_n, _d)] = dict(seed=1300 + _d, d=_d, W=4096, specs=_promotions(_d), order=_o, beta_mu=300.0)
        ARRIVAL_CASES["bursts-%s-d%d" % (_n, _d)] = dict(seed=1400 + _d, d=_d, W=4096, specs=_bursts(_d), order=_o)
        ARRIVAL_CASES["headtail-%s-d%d" % (_n, _d)] = dict(seed=1500 + _d, d=_d, W=4096, specs=_headtail(_d), order=_o)
ARRIVAL_CASES["lens-2048-d6"] = dict(seed=1601, d=6, W=4096, specs=[plain(2048, ("robin", 0)), plain(2047, ("robin", 1)), plain(1, ("robin", 77))])
ARRIVAL_CASES["lens-2049-d14"] = dict(seed=1602, d=14, W=4096, specs=[plain(2049, ("robin", 0)), plain(2047, ("robin", 1))])
ARRIVAL_CASES["lens-2049-d6-large"] = dict(seed=1603, d=6, W=4096, specs=[plain(2049, ("robin", 0)), plain(2047, ("robin", 1))], large=True)
ARRIVAL_CASES["lens-2048-sorted-d6-large"] = dict(seed=1604, d=6, W=4096, large=True, order="sorted",
                                                  specs=[plain(2048, ("robin", 0)), plain(2047, ("robin", 1)), plain(1, ("robin", 77))])
ARRIVAL_CASES["bursts-robin-d14-large"] = dict(seed=1605, d=14, W=4096, specs=_bursts(14), large=True)
ARRIVAL_CASES["headtail-robin-d14-large"] = dict(seed=1606, d=14, W=4096, specs=_headtail(14), large=True)
ARRIVAL_CASES["breath-robin-d14-large"] = dict(seed=1607, d=14, W=4096, specs=_breathing(14), large=True)
ARRIVAL_CASES["breath-sorted-d40-large"] = dict(seed=1608, d=40, W=4096, specs=_breathing(40), large=True, order="sorted")
ARRIVAL_CASES["promo-robin-d6-large"] = dict(seed=1609, d=6, W=4096, specs=_promotions(6), large=True, beta_mu=300.0)
ARRIVAL_CASES["promo-robin-d40"] = dict(seed=1610, d=40, W=4096, specs=_promotions(40), beta_mu=300.0)
for _o in ("period", "sorted", "shuffled"):
    _n = "robin" if _o == "period" else _o
    ARRIVAL_CASES["create-%s-d6" % _n] = dict(seed=1700, d=6, W=4096, specs=_creations(6), order=_o, beta_mu=8.0)
    ARRIVAL_CASES["many-%s-d6" % _n] = dict(seed=1750, d=6, W=4096, specs=_many(6), order=_o)
ARRIVAL_CASES["create-robin-d20-large"] = dict(seed=1701, d=20, W=4096, specs=_creations(20), large=True, beta_mu=8.0)
ARRIVAL_CASES["lens-filter-k3-robin-d14"] = dict(seed=1800, d=14, W=4096, specs=_lens(14), filt=True, k=3.0)
ARRIVAL_CASES["lens-filter-k3-sorted-d14"] = dict(seed=1800, d=14, W=4096, specs=_lens(14), filt=True, k=3.0, order="sorted")
ARRIVAL_CASES["bursts-filter-k3-d14"] = dict(seed=1801, d=14, W=4096, specs=_bursts(14), filt=True, k=3.0)
ARRIVAL_CASES["headtail-filter-k3-d14"] = dict(seed=1802, d=14, W=4096, specs=_headtail(14), filt=True, k=3.0)
# the large windows: 8 191 + 8 192 + 1 and 8 193 + 8 191 members per period of 16 384; one row takes every point of 49 152
ARRIVAL_CASES["w16384-8192-d6"] = dict(seed=1901, d=6, W=16384, specs=[plain(8192, ("robin", 0)), plain(8191, ("robin", 1)), plain(1, ("robin", 99))])
ARRIVAL_CASES["w16384-8193-d6"] = dict(seed=1902, d=6, W=16384, specs=[plain(8193, ("robin", 0)), plain(8191, ("robin", 1))])
ARRIVAL_CASES["w49152-all-d3"] = dict(seed=1903, d=3, W=49152, specs=[plain(49152, ("robin", 0))])
del _d, _o, _n

LARGE_WINDOW = [n for n, kw in ARRIVAL_CASES.items() if kw["W"] > 4096]
W4096 = [n for n in ARRIVAL_CASES if n not in LARGE_WINDOW]


def twin_of(name):
    """The `shuffled` twin of an ordered case (None where the case has none)."""
    for o in ("robin", "sorted"):
        t = name.replace("-%s-" % o, "-shuffled-")
        if t != name and t in ARRIVAL_CASES:
            return t
    return None


def build_arrivals(name):
    return arrivals(**ARRIVAL_CASES[name])


if __name__ == "__main__":  # every case against the oracle alone (no GPU)
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name in sys.argv[1:] or ARRIVAL_CASES:
        t0 = time.time()
        case = build_arrivals(name)
        t1 = time.time()
        res = T.oracle_online(case)
        t2 = time.time()
        T.check_online(case, res)
        print("%-28s ok: %4d + %4d rows, %6d points, paths %s, build %.2f s, oracle %.2f s" % (
            name, len(case[0]), len(case[1]) if case[1] is not None else 0, len(case[3]),
            dict(zip(*[x.tolist() for x in np.unique(res["path"], return_counts=True)])), t1 - t0, t2 - t1))
