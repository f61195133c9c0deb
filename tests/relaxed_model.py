"""A CPU model of the RELAXED multi-GPU mode (cc_comm_set_relaxed), written from DESIGN.md section 6 (3) on top of the CPU
oracle.  TEST INFRASTRUCTURE ONLY.

The mode is not the reference's algorithm, but it is a deterministic one: the super-step schedule depends on the shard
length alone, phase A is the reference's loop without creation on each rank's mini-batch, phase M sums the ranks' CF deltas
in rank order (the in-process transport) and promotes on the merged rows in row order, phase B is the reference's loop over
the set-aside points of all ranks in rank order.  The model states exactly that:

  snapshot  both lists and the two id counters;
  A         per rank a fresh oracle holding the snapshot runs the rank's mini-batch through co_online with creation switched
            off (OracleHDDStream.no_create): a point that nothing absorbs gets uid -1 and path 8 and changes nothing;
  M         per snapshot row and rank delta = local - snapshot of CF1, CF2 and W; the deltas are summed in rank order starting
            from rank 0's; a row whose summed dW is 0 stays as stored (centroid and preference included); every other row
            gets W = w + dW, CF = cf + dCF, cen = CF1 / W, pref = k where CF2 / W - (CF1 / W)^2 <= delta_sq else 1 - numpy's
            elementwise operations are IEEE and uncontracted, as the library's build (-ffp-contract=off) is; kinds and ids are
            the snapshot's; outlier rows that were touched, weigh beta * mu or more and hold at most pi entries above 1 are
            promoted in outlier-list order - consecutive fresh pcore ids, appended to the pcore list;
  B         the set-aside indices of all ranks, in rank order, go through a plain co_online on the merged state.

Outlier-list order is the order of the table's rows: cc_decay_downgrade gathers the rows as pcore list, then outlier list
(k_gather_rows), cc_inject_* and the creation path append a row and a list position together, and a promotion changes a row's
kind where it lies.  `rows` below is the pcore list, then the outlier list, of the snapshot: the table's own order right after
an injection or a timestep boundary (the row ranges of k_rel_promote's threads are then ranges of it), and the same order of
the outlier rows among themselves at any time.

A state is dict(pcore=table, outlier=table, counters=(pcore_last_id, outlier_last_id)), a table what OracleHDDStream.table
returns.  `relaxed_online` returns what the library's handles must hold bit for bit, and per super-step what a test needs to
show that a case exercises what it was built for."""
import ctypes as C

import numpy as np

from oracle import oracle as O

COLS = ("cf1", "cf2", "cen", "pref")


def empty_state(d):
    def t():
        return dict(id=np.zeros(0, np.int64), uid=np.zeros(0, np.int64), w=np.zeros(0), **{c: np.zeros((0, d)) for c in COLS})
    return dict(pcore=t(), outlier=t(), counters=(0, 0))


def state_of(o, d=None):
    """The state an oracle holds."""
    if O.lib().co_dim(o._h) == 0:
        return empty_state(d)
    return dict(pcore=o.table(O.PCORE), outlier=o.table(O.OUTLIER), counters=o.counters)


def oracle_of(par, state, lam=1.0, no_create=False):
    """A fresh oracle with the parameters of `par` (table_util.Params) holding `state`, counters included."""
    o = O.OracleHDDStream(dict(epsilon=1.0, upsilon=1.0, delta=0.5, beta=par.beta, k=par.k, **{"lambda": lam}))
    o.__dict__.update(epsilon_squared=par.eps_sq, delta_squared=par.delta_sq, k=par.k, beta=par.beta, mu=par.mu,
                      omicron=par.omicron, upsilon=par.ups_eps, delta=par.delta, pi=par.pi, lambbda=lam, no_create=no_create)
    assert o.upsilon ** 2 == par.ups_eps_sq
    o._push_params()
    L, dp = O.lib(), C.POINTER(C.c_double)
    for kind, name in ((O.PCORE, "pcore"), (O.OUTLIER, "outlier")):
        t = state[name]
        cols = [np.ascontiguousarray(t[c], dtype=np.float64) for c in COLS]
        d = cols[0].shape[1] if len(t["w"]) else 0
        base = [c.ctypes.data for c in cols]
        for r in range(len(t["w"])):
            ptrs = [C.cast(b + 8 * d * r, dp) for b in base]
            rc = L.co_inject_mc(o._h, kind, d, ptrs[0], ptrs[1], ptrs[2], ptrs[3], float(t["w"][r]), int(t["id"][r]),
                                int(t["uid"][r]))
            assert rc == 0
    o.set_counters(*state["counters"])
    return o


def super_steps(shard, minibatch):
    """[(start, end)] within a shard: mini-batches start at min(minibatch, 2 048) points and double up to `minibatch`; the
    schedule depends on the shard length alone (an empty shard has none: every rank uses the LONGEST shard's schedule)."""
    out, pos, size = [], 0, min(minibatch, 2048)
    while pos < shard:
        out.append((pos, min(shard, pos + size)))
        pos, size = pos + size, min(minibatch, size * 2)
    return out


def _run(o, X):
    n, d = X.shape
    uid, path = np.empty(n, np.int64), np.empty(n, np.int8)
    if n:
        X = np.ascontiguousarray(X, dtype=np.float64)
        rc = O.lib().co_online(o._h, X.ctypes.data_as(C.POINTER(C.c_double)), n, d, uid.ctypes.data_as(C.POINTER(C.c_int64)),
                               path.ctypes.data_as(C.POINTER(C.c_int8)))
        assert rc == 0
    return uid, path


def _rows(state):
    """The snapshot's rows in table order: (uid, w, cf1, cf2, cen, pref, id) of the pcore list, then the outlier list."""
    p, q = state["pcore"], state["outlier"]
    return {key: np.concatenate([p[key], q[key]]) for key in ("uid", "id", "w") + COLS}


def merge(par, snap, locals_):
    """Phase M.  snap: the snapshot state; locals_: the ranks' states after phase A, in rank order.  Returns (the merged
    state, dict(touched, promoted, by_rank: the rows' summed and per-rank dW, ...)) with rows in table order."""
    rows = _rows(snap)
    m, mp = len(rows["w"]), len(snap["pcore"]["w"])
    pos = {int(u): r for r, u in enumerate(rows["uid"])}
    total = None
    dws = []
    for loc in locals_:
        lr = _rows(loc)
        at = np.empty(m, np.int64)
        at[[pos[int(u)] for u in lr["uid"]]] = np.arange(m)      # snapshot row r is the local state's row at[r]
        delta = (lr["cf1"][at] - rows["cf1"], lr["cf2"][at] - rows["cf2"], lr["w"][at] - rows["w"])
        dws.append(delta[2])
        total = delta if total is None else tuple(a + b for a, b in zip(total, delta))   # rank order, from rank 0's value
    d1, d2, dw = total
    touched = dw != 0.0
    w = np.where(touched, rows["w"] + dw, rows["w"])
    cf1 = np.where(touched[:, None], rows["cf1"] + d1, rows["cf1"])
    cf2 = np.where(touched[:, None], rows["cf2"] + d2, rows["cf2"])
    with np.errstate(all="ignore"):
        qa, qb = cf2 / w[:, None], cf1 / w[:, None]
        var = qa - qb * qb
    cen = np.where(touched[:, None], qb, rows["cen"])
    pref = np.where(touched[:, None], np.where(var <= par.delta_sq, par.k, 1.0), rows["pref"])
    beta_mu = par.beta * par.mu
    up = touched & (w >= beta_mu) & ((pref > 1.0).sum(axis=1) <= par.pi)
    up[:mp] = False
    ids = rows["id"].copy()
    promoted = np.flatnonzero(up)                                 # table order = outlier-list order
    pid = snap["counters"][0]
    ids[promoted] = pid + np.arange(len(promoted))
    stay_p = np.arange(mp)
    stay_o = np.array([r for r in range(mp, m) if not up[r]], np.int64)
    order_p = np.concatenate([stay_p, promoted]).astype(np.int64)
    cols = dict(id=ids, uid=rows["uid"], w=w, cf1=cf1, cf2=cf2, cen=cen, pref=pref)
    merged = dict(pcore={k: v[order_p] for k, v in cols.items()}, outlier={k: v[stay_o] for k, v in cols.items()},
                  counters=(pid + len(promoted), snap["counters"][1]))
    info = dict(rows=rows, touched=touched, promoted=promoted, dw=dw, dw_by_rank=dws, w=w, pref=pref, cen=cen, n_pcore=mp,
                heavy=w >= beta_mu)
    return merged, info


def relaxed_online(par, state, X, world, minibatch, lam=1.0):
    """One call of the relaxed online phase on `state` (not modified): dict(uid, path: per point; state: afterwards;
    stats: super_steps, minibatch_points (by rank: cc_relaxed_stats counts a rank's own), deferred_points; steps: per
    super-step dict(ranges, local: [(uid, path)] by rank, info: merge's, deferred: the set-aside indices in the order phase B
    takes them, b: (uid, path) of phase B, before / after: the states around the merge))."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, d = X.shape
    uid, path = np.full(n, -1, np.int64), np.zeros(n, np.int8)
    stats = dict(super_steps=0, minibatch_points=[0] * world, deferred_points=0)
    steps = []
    if n == 0:
        return dict(uid=uid, path=path, state=state, stats=stats, steps=steps)
    shard = -(-n // world)
    for s0, s1 in super_steps(shard, minibatch):
        ranges = []
        for r in range(world):
            a0 = min(n, r * shard)
            e0 = min(n, a0 + shard)
            ranges.append((min(e0, a0 + s0), min(e0, a0 + s1)))
        have_rows = len(state["pcore"]["w"]) + len(state["outlier"]["w"]) > 0
        locals_, local_labels = [], []
        for a, e in ranges:
            if have_rows:
                o = oracle_of(par, state, lam, no_create=True)
                lu, lp = _run(o, X[a:e])
                locals_.append(state_of(o, d))
            else:                                                # an empty table absorbs nothing
                lu, lp = np.full(max(0, e - a), -1, np.int64), np.full(max(0, e - a), 8, np.int8)
            uid[a:e], path[a:e] = lu, lp
            local_labels.append((lu, lp))
        if have_rows:
            merged, info = merge(par, state, locals_)
        else:
            merged, info = state, None
        deferred = np.concatenate([a + np.flatnonzero(lu == -1) for (a, e), (lu, lp) in zip(ranges, local_labels)]).astype(np.int64)
        o = oracle_of(par, merged, lam)
        bu, bp = _run(o, X[deferred]) if len(deferred) else (np.zeros(0, np.int64), np.zeros(0, np.int8))
        if len(deferred):
            uid[deferred], path[deferred] = bu, bp
            after = state_of(o, d)
        else:
            after = merged
        stats["super_steps"] += 1
        for r, (a, e) in enumerate(ranges):
            stats["minibatch_points"][r] += e - a
        stats["deferred_points"] += len(deferred)
        steps.append(dict(ranges=ranges, local=local_labels, info=info, deferred=deferred, b=(bu, bp), before=state,
                          merged=merged, after=after))
        state = after
    return dict(uid=uid, path=path, state=state, stats=stats, steps=steps)


def params_of(o):
    """table_util.Params of an OracleHDDStream whose dataset-dependent parameters are set."""
    from table_util import Params
    return Params(o.epsilon_squared, o.delta_squared, o.k, o.beta, float(o.mu), float(o.omicron), o.upsilon, o.upsilon ** 2,
                  o.delta, int(o.pi))


def relaxed_stream(config, Xs, daystamps, world, minibatch):
    """HDDStream.online_microcluster_maintenance per timepoint as a relaxed group runs it: the reference's parameter
    derivation and decay / downgrade / deletion at the boundary (the oracle's), the relaxed online phase (the model), the
    offline phase on the model's table (the oracle's).  Per timepoint what relaxed_online returns plus `members`, every final
    cluster's pcore ids in merge order, and `boundary`, how many rows the boundary before it downgraded and deleted."""
    ref = O.OracleHDDStream(config)                           # (parameters and the timestamp only; it never holds a row)
    state, out = None, []
    for X, day in zip(Xs, daystamps):
        X = np.ascontiguousarray(X, dtype=np.float64)
        ref.set_dataset_dependent_parameters(X)
        par = params_of(ref)
        if state is None:
            state = empty_state(X.shape[1])
        if ref.last_data_timestamp - day != 0:
            o = oracle_of(par, state, ref.lambbda)
            O.lib().co_decay_downgrade(o._h, 2 ** (-ref.lambbda * (day - ref.last_data_timestamp)))
            before, state = state, state_of(o, X.shape[1])
            gone = set(before["pcore"]["uid"].tolist()) - set(state["pcore"]["uid"].tolist())
            boundary = dict(downgraded=len(gone & set(state["outlier"]["uid"].tolist())),
                            deleted=sum(len(before[k]["w"]) - len(state[k]["w"]) for k in ("pcore", "outlier")))
        else:
            boundary = dict(downgraded=0, deleted=0)
        res = relaxed_online(par, state, X, world, minibatch, ref.lambbda)
        res["boundary"] = boundary
        ref.last_data_timestamp = day
        state = res["state"]
        o = oracle_of(par, state, ref.lambbda)
        o.offline_clustering()
        res["members"] = [[int(x) for x in c["members"]] for c in o.clusters]
        out.append(res)
    return out
