"""The timestep boundary (cc_decay_downgrade: k_decay, k_downgrade_flags, the host walk over the two lists,
k_gather_rows) against the CPU oracle on injected pcore and outlier lists.

The decay factor is 2^-lambda with lambda = 1, so `w * f` is exact and weights can sit ON the thresholds:
w * f == beta * mu stays a pcore (the test is `<`), w * f == omicron is deleted (the test is `<=`).  The lists hold runs
of 1 to 5 consecutive flagged rows (Python removes from the list it iterates, so the row that slides into a freed
position is skipped: every second row of a run survives), pcores that are downgraded and deleted in the same call,
pcores flagged only because more than pi of their stored preference entries exceed 1, and tables that empty
completely.  The call is applied twice - the second one starts from what k_gather_rows wrote - and followed by an
offline phase on both sides.  Both lists (order included: id, uid, w, cf1, cf2, cen, pref), the id counters and the
offline results are compared for bit equality."""
import numpy as np
import pytest

import table_util as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

F = 2.0 ** -1.0          # lambda = 1
BETA, MU, OMICRON = 0.5, 4.0, 0.25


def _runs(rng, m):
    """Flags in runs of 1, 2, 3, 4, 5, 1, ... separated by one or two unflagged rows."""
    flags, r = [], 1
    while len(flags) < m:
        flags += [True] * r + [False] * int(rng.integers(1, 3))
        r = r % 5 + 1
    return np.array(flags[:m], dtype=bool)


def boundary_lists(seed, m_p, m_o, d):
    """(pcores, outliers, params): centroids in groups of ~4 (jitter 0.02 around centres in [0, 10)^d)."""
    rng = np.random.default_rng(seed)
    pi = d - 2 if d >= 3 else d
    k = 4.0

    def cen(m):
        return rng.uniform(0.0, 10.0, (m // 4 + 1, d))[np.arange(m) // 4] + rng.normal(0.0, 0.02, (m, d))

    def pref(m, over):
        p = np.ones((m, d))
        for r in range(m):
            n = d if over[r] else int(rng.integers(0, pi + 1))
            p[r, rng.choice(d, n, replace=False)] = k
        return p

    # pcores: unflagged ones weigh 4 (exactly beta * mu after the decay: stays) or more
    flag = _runs(rng, m_p)
    how = rng.integers(0, 4 if pi < d else 3, m_p)
    w = np.where(rng.random(m_p) < 0.3, 4.0, rng.uniform(4.5, 40.0, m_p))
    sel = flag & (how == 0)
    w[sel] = rng.uniform(0.6, 3.9, int(sel.sum()))          # downgraded, survives as an outlier
    sel = flag & (how == 1)
    w[sel] = rng.uniform(0.1, 0.5, int(sel.sum()))          # downgraded and deleted in the same call
    sel = flag & (how == 2)
    w[sel] = 0.5                                            # ... at w * f == omicron exactly
    over = flag & (how == 3)                                # flagged by count(pref > 1) > pi alone
    pcores = T.Table(cen(m_p), rng.uniform(0.0, 1e-4, (m_p, d)) / d, pref(m_p, over), w,
                     rng.permutation(m_p) + 10, rng.permutation(m_p) + 100_000)
    # outliers: flagged ones weigh 0.5 (exactly omicron after the decay: deleted) or less
    flag = _runs(rng, m_o)
    w = np.where(rng.random(m_o) < 0.3, 0.5 * (1.0 + 2.0 ** -52), rng.uniform(0.6, 10.0, m_o))
    w[flag] = np.where(rng.random(int(flag.sum())) < 0.5, 0.5, rng.uniform(0.01, 0.5, int(flag.sum())))
    outliers = T.Table(cen(m_o), rng.uniform(0.0, 1e-4, (m_o, d)) / d, pref(m_o, np.zeros(m_o, bool)), w,
                       rng.permutation(m_o) + 200_000, rng.permutation(m_o) + 200_000)
    ups_eps = 0.06 * float(np.sqrt(d))
    par = T.Params(0.03 ** 2, 0.05 ** 2, k, BETA, MU, OMICRON, ups_eps, ups_eps ** 2, 0.05, pi)
    return pcores, outliers, par


def _both(par, pcores, outliers):
    from chronoclust_amd import _lib
    h = T.fill_handle(_lib.Handle(0), par, pcores, outliers)
    o = T.make_oracle(par, pcores, outliers)
    return h, o


def _flagged(tab, par):
    return (tab["w"] < par.beta * par.mu) | ((tab["pref"] > 1.0).sum(axis=1) > par.pi)


def _offline_after(h, o, par, what):
    """The offline phase on what the boundary left, with pi = d and a low mu so that clusters form."""
    par2 = par._replace(pi=h.dim() if h.dim() > 0 else par.pi, mu=0.5)
    h.set_params(*par2)
    o.pi, o.mu = par2.pi, par2.mu
    exp = T.oracle_offline(o)
    T.same_offline(T.handle_offline(h), exp, what)
    return exp


# (pcores, outliers, d): m = 1, 255, 256, 257 and 50 000 rows in all; d at and off the compiled widths
SHAPES = [(1, 1, 3), (200, 55, 8), (128, 128, 13), (257, 0, 20), (0, 257, 21), (150, 106, 41), (100, 155, 64),
          (129, 128, 65), (56, 200, 129), (155, 100, 300), (255, 2, 1), (30_000, 20_000, 5)]


@pytest.mark.parametrize("m_p,m_o,d", SHAPES)
def test_decay_downgrade_against_oracle(m_p, m_o, d):
    pcores, outliers, par = boundary_lists(1000 * d + m_p, m_p, m_o, d)
    h, o = _both(par, pcores, outliers)
    T.same_lists(h, o, "injected")
    for call in (1, 2):
        before_p, before_o = o.table(0), o.table(1)
        T.oracle_lib().co_decay_downgrade(o._h, F)
        h.decay_downgrade(F)
        T.same_lists(h, o, "after call %d" % call)
        op, oo = o.table(0), o.table(1)
        if call == 1 and m_p >= 100:
            # the structure is there, by the oracle's lists: thresholds met exactly on both sides of each test, flagged
            # pcores that the walk skipped, pcores that were downgraded and deleted at once, rows flagged by pi alone
            assert (op["w"] == BETA * MU).any() and _flagged(op, par).any()
            gone = set(before_p["uid"].tolist()) - set(op["uid"].tolist()) - set(oo["uid"].tolist())
            assert len(gone) > 0
            if par.pi < d:
                assert ((before_p["w"] * F >= BETA * MU) & ((before_p["pref"] > 1.0).sum(axis=1) > par.pi)).any()
        if call == 1 and m_o >= 100:
            assert (before_o["w"] * F == OMICRON).any() and (oo["w"] <= OMICRON).any()  # (deleted at equality; skipped)
            assert (oo["w"] == OMICRON * (1.0 + 2.0 ** -52)).any()
    exp = _offline_after(h, o, par, "offline after the boundary")
    if m_p >= 100:
        assert max(len(c["members"]) for c in exp[1]) > 1
    h.close()


def test_single_pcore_downgraded_and_deleted_empties_the_table():
    """m = 1: the pcore falls below beta * mu and below omicron in one call - no row is left (no gather is launched);
    the next call and the offline phase see an empty table, and an injection afterwards starts a new list."""
    pcores, _, par = boundary_lists(5, 1, 0, 5)
    pcores.w[:] = 0.4
    pcores = T.Table(pcores.cen, 1e-5, pcores.pref, pcores.w, pcores.id, pcores.uid)
    h, o = _both(par, pcores, None)
    for call in (1, 2):
        T.oracle_lib().co_decay_downgrade(o._h, F)
        h.decay_downgrade(F)
        assert len(o.table(0)["id"]) == 0 and len(o.table(1)["id"]) == 0
        assert h.count(0) == 0 and h.count(1) == 0 and h.counters() == o.counters
    exp = T.oracle_offline(o)
    got = T.handle_offline(h)
    assert len(got[1]) == len(exp[1]) == 0 and got[0]["num_core"] == 0
    more, _, _ = boundary_lists(6, 9, 0, 5)
    T.fill_handle(h, par, more)
    for r in range(len(more)):
        o.inject(0, more.cf1[r], more.cf2[r], more.cen[r], more.pref[r], more.w[r], more.id[r], more.uid[r])
    T.same_lists(h, o, "refilled")
    h.close()


@pytest.mark.parametrize("m_p,m_o,d", [(7, 0, 4), (64, 33, 24), (300, 300, 16)])
def test_repeated_calls_empty_the_table(m_p, m_o, d):
    """Every row flagged on both lists: each call keeps every second row of what is left; compared after every call
    until nothing is left."""
    pcores, outliers, par = boundary_lists(77 + d, m_p, m_o, d)
    pcores = T.Table(pcores.cen, 1e-5, pcores.pref, np.full(m_p, 0.3), pcores.id, pcores.uid)
    outliers = T.Table(outliers.cen, 1e-5, outliers.pref, np.full(m_o, 0.2), outliers.id, outliers.uid)
    h, o = _both(par, pcores, outliers if m_o else None)
    calls = 0
    while len(o.table(0)["id"]) + len(o.table(1)["id"]) > 0:
        T.oracle_lib().co_decay_downgrade(o._h, F)
        h.decay_downgrade(F)
        calls += 1
        T.same_lists(h, o, "after call %d" % calls)
        assert calls < 40
    assert calls >= 3 and h.count(0) == 0 and h.count(1) == 0
    h.close()
