"""Designed inputs for the SEQUENTIAL kernels of the online phase (csrc/cc_seq_r.h: k_seq_r, the table in registers, d = 2 .. 4;
cc_seq.h: k_seq, the table in LDS; cc_seq_g.h: k_seq_g, the table in HBM, narrow up to 128 dimensions and wide up to 1 024) and
for the hand-over between them (cc_online_run.h: sequential_stint; cc_policy.h: SeqHandover): tables and streams that sit ON the
kernels' constants - k_seq_r's 64 pcore slots and 64 QO outlier slots (QO = 4 at d <= 3, 3 at d = 4), the `n_lanes <= 16`
shortcut of its minimum, k_seq's image of 6600 / (4 d + 5) rows and its staged chunk of min(64, 512 / d) points, k_seq_g's stride
of 1 024 threads, its sixteen waves, its chunk of 512 / d (narrow) or 1 024 / d (wide) points, the switches at 128 / 129 and
512 / 513 dimensions, and the host's chunk of 8 192 points.

The geometry is trivial and every number dyadic.  Rows sit on sites 4 apart in dimensions 0 and 1 (a point of one site is refused by
every row of another: tentative variance 16 w / (w + 1)^2), variances are 0 (with the pdim filter: 1/1024 in the last two dimensions,
entries 1 there), stored entries are k where the variance says so: a handle stays untainted.  eps^2 = 1/256, delta^2 = 1/4096,
beta mu = 8, pcore rows weigh 7 (a few 15), outlier rows 3, promotable ones beta mu - 1 = 7.  A stream is written event by event:

  join      a point ON a row's centroid: distance 0, the centroid stays where it is (c (w + 1) / (w + 1) is exact), every entry
            stays what it is - the row can be used again;
  promote   the same on an outlier row of weight 7: path 5, the row gets the next pcore id and the next pcore key;
  create    a point on a fresh site: path 2, the row gets the next outlier id;
  tie       two or three rows 1/8 from the point along different axes or on either side of it (rows of a pair are 1/4 apart):
            equal distances, equal bit for bit - the smallest list-order key wins, the tentative variance 1/64 w / (w + 1)^2 is
            above delta^2 and its term below eps^2, so the winner absorbs the point (its centroid moves: a row that won a tie is
            not used again).  A row 1/4 from a point refuses it at weight 7 (7/1024 > eps^2) and accepts at weight 15
            (15/4096 < eps^2): a tie between two such rows ends differently by who wins.

So the uid and the path of EVERY point are known when the case is written (meta["uid"], meta["path"]), and so are the list sizes
around every promotion and creation (meta["events"]), the rows tied for a point (meta["ties"]) and what each sequential kernel is
meant to take (meta["shares"], written from the event indices - not from the model below).  `check_seq_edge` asserts all of it on
the ORACLE's result alone.  The `g-dims` cases without filter are table_util.lattice as it stands (ties and radii exactly on
eps^2); its filter + k = 3 variants are written here, since the lattice thresholds (delta^2 > eps^2) leave the filter nothing to
admit.

No goldens of the Python reference accompany these cases: it cannot be imported where the suite is built, and the oracle - pinned
to the reference elsewhere - is the referee.

The hand-over model: `model_shares`, see its docstring."""
import numpy as np

import table_util as T
from table_util import Params

EPS_SQ, DELTA_SQ, BETA, MU = 1.0 / 256.0, 1.0 / 4096.0, 0.5, 16.0
WIDE_VAR = 1.0 / 1024.0          # with the pdim filter: the variance of a row's last two dimensions (entries 1 there)
TIE = 1.0 / 8.0                  # a tied row's distance from its point; the rows of a pair are 2 TIE apart
HOST_CHUNK = 8192                # sequential_stint's chunk
SEQ_DOUBLES = 6600               # CC_SEQ_DOUBLES: k_seq's LDS image
WINDOW_MAX_DIM = 64


def seq_cap_rows(d):
    """cc_seq_cap_rows (cc_host.h): rows of k_seq's LDS image."""
    return SEQ_DOUBLES // (4 * d + 5)


def seq_r_qo(d):
    """SeqRShape<D>::QO (cc_seq_r.h): outlier slots per lane."""
    return 4 if d <= 3 else 3


def seq_chunk(d):
    """Points k_seq stages at a time."""
    return min(64, 512 // d)


def seq_g_chunk(d):
    """Points k_seq_g stages at a time: narrow up to 128 dimensions, wide beyond (one point beyond 512)."""
    return min(64, 512 // d) if d <= 128 else max(1, 1024 // d)


# ---- the hand-over model ------------------------------------------------------------------------------------------------

MODES = {
    "seq2": {},
    "seq2-seqr0": dict(CHRONOCLUST_HIP_SEQR=0),
    "seq2-seqg0": dict(CHRONOCLUST_HIP_SEQG=0),
}


def model_shares(case, paths, env):
    """Who takes which points of a call with set_tuning(sequential=2) on a fresh handle that holds the case's lists: plain Python
    over the sizes of the initial lists and the oracle's per-point path codes (0 pcore join, low bits 1 outlier join, 5 join with
    promotion, 2 creation).  Returns dict(seq_points, seq_r_points, seq_g_points, window_points) as cc_stats counts them:
    seq_points is what ALL three kernels took (each adds to Ctl::stat_seq_points), seq_r_points and seq_g_points are parts of it.
    env: the knobs around the handle's creation (CHRONOCLUST_HIP_SEQR / _SEQG = 0).

    Written from the header comments of cc_seq_r.h / cc_seq.h / cc_seq_g.h, OnlineRun::sequential_stint and SeqHandover:
      1. The call proceeds in stints of at most 8 192 points; a stint starts where the previous one stopped.
      2. A stint goes to k_seq_g if the table holds cap(d) = 6600 / (4 d + 5) rows or more at its start and k_seq_g is allowed
         (seq_g_applies), always beyond 64 dimensions.  k_seq_g takes the whole stint: it stops only when the table's capacity is
         used up, and the host reserves 8 192 rows ahead of every stint.
      3. With cap(d) rows or more and k_seq_g forbidden no sequential kernel is possible (seq_possible): the windows take the rest
         of the call - rows are never deleted during a call, so nothing brings the sequential kernels back.
      4. Else k_seq_r runs first where d is 2 .. 4 and it is allowed.  At load it takes nothing unless M <= 64 + 64 QO, n_p <= 64
         and n_o <= 64 QO.  Before every point it stops if n_p >= 64 or n_o(at load) + creations since load >= 64 QO: promotions
         do not free a slot within a stint (every stint loads the rows anew, so burnt slots come back).
      5. k_seq, launched behind it, takes what k_seq_r left of the stint (Ctl::seq_rest) and stops before the creation that finds
         M >= cap(d); the next stint starts at that point (rule 2 or 3 then applies).
    Where the issue that asked for this model and the code differ: none of the rules; one wording - `r-reload`'s sixth creation
    would not itself be refused without the reload (255 slots are in use before it: it takes the last one), the points AFTER it
    would be."""
    pcores, outliers, par, X, meta = case
    n, d = X.shape
    n_p = len(pcores) if pcores is not None else 0
    n_o = len(outliers) if outliers is not None else 0
    M = n_p + n_o
    allow_r = str(env.get("CHRONOCLUST_HIP_SEQR", 1)) != "0"
    allow_g = str(env.get("CHRONOCLUST_HIP_SEQG", 1)) != "0"
    cap = 0 if d > WINDOW_MAX_DIM else seq_cap_rows(d)
    qo = seq_r_qo(d)
    out = dict(seq_points=0, seq_r_points=0, seq_g_points=0, window_points=0)

    def apply(code):
        nonlocal n_p, n_o, M
        if code == 2:
            n_o, M = n_o + 1, M + 1
        elif code == 5:
            n_p, n_o = n_p + 1, n_o - 1
        else:
            assert code in (0, 1), code

    pos = 0
    while pos < n:
        stint = [int(c) for c in paths[pos:pos + HOST_CHUNK]]
        if M >= cap:
            if not allow_g:
                assert d <= WINDOW_MAX_DIM
                out["window_points"] = n - pos
                break
            for code in stint:
                apply(code)
            out["seq_points"] += len(stint)
            out["seq_g_points"] += len(stint)
            pos += len(stint)
            continue
        i = 0
        if allow_r and 2 <= d <= 4 and M <= 64 + 64 * qo and n_p <= 64 and n_o <= 64 * qo:
            slots = n_o
            while i < len(stint) and n_p < 64 and slots < 64 * qo:
                apply(stint[i])
                slots += stint[i] == 2
                i += 1
            out["seq_r_points"] += i
        while i < len(stint) and not (stint[i] == 2 and M >= cap):
            apply(stint[i])
            i += 1
        out["seq_points"] += i
        pos += i
        assert i > 0 or M >= cap          # (a stint that takes nothing has a full image: rule 2 or 3 is next)
    return out


# ---- writing a case event by event --------------------------------------------------------------------------------------

class _Row(object):
    __slots__ = ("kind", "idx", "cen", "w", "w0", "uid", "key", "moved", "injected")

    def __init__(self, kind, idx, cen, w):
        self.kind, self.idx, self.cen, self.w, self.w0 = kind, idx, cen, w, w
        self.uid, self.key, self.moved, self.injected = None, idx, False, True


class _Design(object):
    """Rows first (pcore / outlier / place), then `seal`, then the stream (join / promote / create / tie)."""

    def __init__(self, seed, d, k=4.0, filt=False):
        assert d >= 2 and (not filt or d >= 4)
        self.rng = np.random.default_rng(seed)
        self.d, self.k, self.filt = d, float(k), filt
        self.rows = {"p": [], "o": []}
        self._sites = 0
        self.sealed = False

    def site(self):
        i = self._sites
        self._sites += 1
        c = np.zeros(self.d)
        c[0], c[1] = 4.0 * (i % 64), 4.0 * (i // 64)
        return c

    def axis(self, i, s=1.0):
        e = np.zeros(self.d)
        e[i] = s
        return e

    def pcore(self, w=7.0, cen=None):
        r = _Row("p", len(self.rows["p"]), self.site() if cen is None else cen, float(w))
        self.rows["p"].append(r)
        return r

    def outlier(self, w=3.0, cen=None):
        r = _Row("o", len(self.rows["o"]), self.site() if cen is None else cen, float(w))
        self.rows["o"].append(r)
        return r

    def fill(self, m_p, m_o, promotable=()):
        """Rows up to m_p pcores and m_o outliers, each on a site of its own; outliers at list positions `promotable` weigh 7."""
        while len(self.rows["p"]) < m_p:
            self.pcore()
        while len(self.rows["o"]) < m_o:
            self.outlier(7.0 if len(self.rows["o"]) in promotable else 3.0)

    def place(self, rows, offsets, centre=None):
        """Moves rows (still untouched) onto `centre` + offset each: the rows of a tie.  Returns the centre."""
        assert not self.sealed
        centre = self.site() if centre is None else centre
        for r, off in zip(rows, offsets):
            r.cen = centre + off
            r.w0 = r.w                      # (weights are final here: the callers set them before placing)
        return centre

    def seal(self):
        d, k = self.d, self.k
        tabs = []
        for kind in ("p", "o"):
            rows = self.rows[kind]
            m = len(rows)
            if m == 0:
                tabs.append(None)
                continue
            cen = np.array([r.cen for r in rows])
            var = np.zeros((m, d))
            pref = np.full((m, d), k)
            if self.filt:
                var[:, d - 2:] = WIDE_VAR
                pref[:, d - 2:] = 1.0
            w = np.array([r.w for r in rows])
            t = T._table(self.rng, cen, var, pref, w) if kind == "p" else T._outlier_table(self.rng, cen, var, pref, w)
            for r in rows:
                r.uid = int(t.uid[r.idx])
            tabs.append(t)
        self.pcores, self.outliers = tabs
        self.n_p, self.n_o = len(self.rows["p"]), len(self.rows["o"])
        self.next_pkey, self.next_okey = self.n_p, self.n_o
        self.next_uid = max([int(t.uid.max()) for t in tabs if t is not None] + [-1]) + 1
        self.pts, self.uid, self.path, self.events, self.ties = [], [], [], [], []
        self.sealed = True
        return self

    @property
    def at(self):
        return len(self.pts)

    def _emit(self, x, uid, path):
        self.pts.append(np.array(x, dtype=np.float64))
        self.uid.append(int(uid))
        self.path.append(int(path))

    def _absorb(self, row, x):
        """Row `row` absorbs x: the point's expected label; a promotion where an outlier reaches beta mu."""
        row.w += 1.0
        if row.kind == "o" and row.w >= BETA * MU:
            self.events.append(dict(at=self.at, what="promotion", uid=row.uid, n_p=(self.n_p, self.n_p + 1),
                                    n_o=(self.n_o, self.n_o - 1)))
            self._emit(x, row.uid, 5)
            row.kind, row.key = "p", self.next_pkey
            self.next_pkey += 1
            self.n_p, self.n_o = self.n_p + 1, self.n_o - 1
        else:
            self._emit(x, row.uid, 0 if row.kind == "p" else 1)

    def join(self, row):
        assert not row.moved, "a row that won a tie is not where it was"
        if self.filt and row.injected:     # (the wide variance after the add, WIDE_VAR w0 / (w + 1), stays above delta^2)
            assert row.w + 1.0 < 4.0 * row.w0, "the filter's wide variance would fall to delta^2"
        self._absorb(row, row.cen)

    def promote(self, row):
        assert row.kind == "o" and row.w == BETA * MU - 1.0
        self.join(row)
        assert row.kind == "p"

    def create(self):
        r = _Row("o", None, self.site(), 1.0)
        r.uid, r.key, r.injected = self.next_uid, self.next_okey, False
        self.events.append(dict(at=self.at, what="creation", uid=r.uid, n_p=(self.n_p, self.n_p), n_o=(self.n_o, self.n_o + 1)))
        self._emit(r.cen, r.uid, 2)
        self.next_uid += 1
        self.next_okey += 1
        self.n_o += 1
        return r

    def tie(self, x, rows, absorbed=True, then=None):
        """A point tied between `rows` (one list, none of them moved): the smallest key wins.  absorbed: the winner takes the
        point; else it refuses (the point is `then`'s, a row of the other list that holds it at distance 0, or a new row's)."""
        assert len({r.kind for r in rows}) == 1 and not any(r.moved for r in rows)
        win = min(rows, key=lambda r: r.key)
        self.ties.append(dict(at=self.at, stage=win.kind, rows=[(r.uid, r.cen.copy()) for r in rows], winner=win.uid,
                              absorbed=absorbed, lose_w=[r.w for r in rows if r is not win], win_w=win.w))
        if absorbed:
            self._absorb(win, x)
            win.moved = True
        elif then is not None:
            self._absorb(then, x)
        else:
            raise ValueError("a refused tie needs the row that takes the point")

    def case(self, name, shares, **more):
        par = Params(EPS_SQ, DELTA_SQ, self.k, BETA, MU, 0.1, 0.5, 0.25, 1.0 / 32.0, self.d - 2 if self.filt else self.d)
        meta = dict(kind="seq-edge", name=name, tainted=False, uid=np.array(self.uid, np.int64), path=np.array(self.path, np.int8),
                    events=self.events, ties=self.ties, shares=shares, **more)
        return self.pcores, self.outliers, par, np.ascontiguousarray(np.array(self.pts)), meta


def _shares(n, r=0, g=0, stop=None, r_possible=True):
    """meta["shares"] of a case of n points: k_seq_r takes r (where it runs), the LDS kernels stop at point `stop` (None: never)
    and k_seq_g takes g = n - stop where allowed (g: given for the cases that start on it)."""
    if stop is not None:
        g = n - stop
    lds = n - g
    out = {"seq2": dict(seq_points=n, seq_r_points=r, seq_g_points=g, window_points=0),
           "seq2-seqg0": dict(seq_points=lds, seq_r_points=min(r, lds), seq_g_points=0, window_points=g)}
    if r_possible:
        out["seq2-seqr0"] = dict(seq_points=n, seq_r_points=0, seq_g_points=g, window_points=0)
    return out


# ---- R: k_seq_r ---------------------------------------------------------------------------------------------------------

def r_lanes16(seed, d):
    """16 pcores, 8 promotable outliers.  c: rows 0 and 15 sit 1/4 from it along axes 0 and 1, row 15 weighs 15, outlier P0 sits
    ON it.  With 16 lanes (the shortcut of cc_seqr_min): a point tied between rows 1 / 14, absorbed; the point on c, tied between
    rows 0 / 15 - row 0 wins and refuses (row 15 would accept), P0 takes it and becomes the 17th pcore, lane 16.  With 17: points
    tied between lane 16 and lane 0, lane 16 and lane 15 - the older row wins both.  Then two outliers 1/4 apart are promoted
    in the order AGAINST their rows (keys 17 and 18 to rows 5 and 2) and joins fill the stint; behind point 8 192 the rows are
    loaded anew in row order, lane 17 holds key 18, lane 18 key 17, and the point tied between them is the smaller KEY's, not the
    smaller lane's."""
    D = _Design(seed, d)
    D.fill(16, 8, promotable=range(8))
    p, o = D.rows["p"], D.rows["o"]
    p[15].w = 15.0
    c = D.place([p[0], p[15], o[0]], [D.axis(0, 2 * TIE), D.axis(1, 2 * TIE), 0.0])
    m = D.place([p[1], p[14]], [D.axis(0, -TIE), D.axis(0, TIE)])
    q = D.place([o[5], o[2]], [D.axis(0, -TIE), D.axis(0, TIE)])
    D.seal()
    D.join(p[7])
    D.tie(m, [p[1], p[14]])
    new0 = D.create()
    D.tie(c, [p[0], p[15]], absorbed=False, then=o[0])           # -> the 17th pcore
    at17 = D.at - 1
    D.tie(c + D.axis(0, TIE), [p[0], o[0]])
    D.tie(c + D.axis(1, TIE), [p[15], o[0]])
    D.promote(o[5])
    D.promote(o[2])
    D.join(new0)
    while D.at < HOST_CHUNK:
        D.join(p[2 + D.at % 12])                                    # rows 2 .. 13: never part of a tie
    D.join(o[0])
    D.tie(q, [o[5], o[2]])
    reload_tie = D.at - 1
    D.create()
    D.join(p[3])
    n = D.at
    return D.case("r-lanes16-d%d" % d, _shares(n, r=n), pcore17_at=at17, reload_tie_at=reload_tie)


def r_p63(seed, d, m_p=63, at=None):
    """m_p pcores and 8 outliers.  m_p = 63: joins, then the promotion that makes the 64th pcore at point `at` - k_seq_r takes
    at + 1 points and stops, k_seq behind it numbers the next promotion and the next creation from the counters it left.  64
    pcores: full at load, nothing taken; 65: the table does not fit."""
    D = _Design(seed, d)
    D.fill(m_p, 8, promotable=(0, 1, 5))
    D.seal()
    p, o = D.rows["p"], D.rows["o"]
    if at is None:
        r = 0
        D.join(p[0]); D.create(); D.promote(o[0]); D.join(o[0]); D.join(o[3]); D.join(p[m_p - 1])
    else:
        r = at + 1
        made = None
        while D.at < at:
            if D.at == 2 and at >= 8:
                made = D.create()
            elif D.at == 5 and at >= 8:
                D.join(o[3])
            else:
                D.join(p[D.at % m_p])
        D.promote(o[0])
    D.join(o[0])
    made2 = D.create()
    D.promote(o[1])
    D.join(made2)
    D.join(o[1])
    D.join(o[4])
    D.create()
    for i in range(22):
        D.join(p[(7 * i) % m_p])
    n = D.at
    name = "r-p63-at%d-d%d" % (at, d) if at is not None else "r-p%d-d%d" % (m_p, d)
    return D.case(name, _shares(n, r=r), pcore64_at=at)


def r_o_fill(seed, d):
    """64 QO - 2 outliers and 5 pcores.  Five promotions (rows on the slot and lane edges): the outlier count falls to 64 QO - 7,
    the slots in use stay 64 QO - 2.  Two creations fill them; the point behind the second one, a plain pcore join, is k_seq's."""
    qo = seq_r_qo(d)
    m_o = 64 * qo - 2
    prom = (0, 63, 64, 127, m_o - 1)
    D = _Design(seed, d)
    D.fill(5, m_o, promotable=prom)
    D.seal()
    p, o = D.rows["p"], D.rows["o"]
    for j in prom:
        D.promote(o[j])
    a = D.create()
    D.create()
    stop = D.at
    D.join(p[2])
    D.join(o[63])
    D.join(a)
    D.create()
    D.join(o[100])
    D.join(p[4])
    n = D.at
    return D.case("r-o-fill-d%d" % d, _shares(n, r=stop), stop_at=stop)


def r_o_full(seed, d, m_o):
    """All 64 QO outlier slots taken at load (d = 2: 256), or one row too many (d = 4: 193): k_seq_r takes nothing."""
    D = _Design(seed, d)
    D.fill(5, m_o, promotable=(1, m_o - 1))
    D.seal()
    p, o = D.rows["p"], D.rows["o"]
    D.join(p[0]); D.promote(o[m_o - 1]); a = D.create(); D.join(o[m_o - 1]); D.join(a); D.promote(o[1]); D.join(o[64]); D.create()
    D.join(p[4])
    n = D.at
    name = "r-o-full-d%d" % d if m_o == 64 * seq_r_qo(d) else "r-o-over-d%d" % d
    return D.case(name, _shares(n, r=0))


def r_slot_ties(seed, d):
    """200 outliers (three slots and part of a fourth), 4 pcores.  Points tied among rows t, t + 64, t + 128 (one lane, three
    slots: the lane's own comparison), between lanes 15 / 16, 31 / 32, 47 / 48 (the rows of the DPP minimum) and between a HIGHER
    slot of a LOWER lane and slot 0 of the next lane (rows 81 / 18, 162 / 35: the smaller key sits in the higher lane).  Rows of
    weight 3 join, rows of weight 7 are promoted out of the tie."""
    heavy = (15, 16, 81, 18, 7, 71, 135)
    D = _Design(seed, d)
    D.fill(4, 200, promotable=heavy)
    p, o = D.rows["p"], D.rows["o"]
    pairs = [(15, 16), (32, 31), (47, 48), (81, 18), (162, 35), (199, 136)]
    triples = [(3, 67, 131), (135, 71, 7)]
    centres = {}
    for a, b in pairs:
        centres[(a, b)] = D.place([o[a], o[b]], [D.axis(0, -TIE), D.axis(0, TIE)])
    for t in triples:
        centres[t] = D.place([o[i] for i in t], [D.axis(0, -TIE), D.axis(0, TIE), D.axis(1, TIE)])
    D.seal()
    D.join(p[1])
    for key in pairs[:3] + triples[:1] + pairs[3:] + triples[1:]:
        D.tie(centres[key], [o[i] for i in key])
        D.join(o[100 + D.at])
    a = D.create()
    D.join(a)
    D.join(p[3])
    n = D.at
    return D.case("r-slot-ties-d%d" % d, _shares(n, r=n))


def r_reload(seed, d):
    """8 192 + 65 points on 250 outliers and 10 pcores: four promotions and five creations in the first stint (the last creation
    ON its last point) use 255 of the 256 slots though 251 outliers remain; the second stint loads them anew, takes the sixth
    creation and every point behind it.  Without the reload the points behind that creation would be k_seq's."""
    D = _Design(seed, d)
    prom = (0, 64, 128, 249)
    D.fill(10, 250, promotable=prom)
    D.seal()
    p, o = D.rows["p"], D.rows["o"]
    made = []
    plan = {1: "c", 2: "p0", 70: "c", 71: "p1", 4000: "c", 4001: "p2", 8189: "c", 8190: "p3", 8191: "c"}
    while D.at < HOST_CHUNK:
        what = plan.get(D.at)
        if what == "c":
            made.append(D.create())
        elif what:
            D.promote(o[prom[int(what[1])]])
        elif D.at % 3 == 0 and D.at < 3 * 63 * 4:
            D.join(o[1 + (D.at // 3) % 63])                         # (four joins each: weight 7, one short of a promotion)
        else:
            D.join(p[D.at % 10])
    assert sum(e["what"] == "promotion" for e in D.events) == 4 and sum(e["what"] == "creation" for e in D.events) == 5
    for i in range(65):
        if i == 10:
            made.append(D.create())
        elif i in (3, 20):
            D.join(made[-1])
        elif i % 2:
            D.join(o[prom[i % 4]])
        else:
            D.join(p[i % 10])
    n = D.at
    assert n == HOST_CHUNK + 65
    return D.case("r-reload-d%d" % d, _shares(n, r=n), sixth_creation_at=HOST_CHUNK + 10)


def r_l_g(seed, d):
    """60 pcores and 190 outliers at d = 4 (192 slots, an image of 314 rows); creations at every even point, 70 in all.  k_seq_r
    takes the first two and stops before point 3, k_seq takes the next 62 (314 rows) and stops before the 65th at point 128,
    k_seq_g takes that one and the rest."""
    assert d == 4
    D = _Design(seed, d)
    D.fill(60, 190, promotable=(0, 189))
    D.seal()
    p, o = D.rows["p"], D.rows["o"]
    made = []
    for i in range(70):
        made.append(D.create())
        if i == 10:
            D.promote(o[189])
        elif i == 66:
            D.promote(o[0])
        elif i % 3 == 0:
            D.join(made[i // 2])
        else:
            D.join(p[i % 60])
    n = D.at
    stop = 2 * (seq_cap_rows(d) - 250)
    assert stop == 128 and n == 140
    return D.case("r-l-g-d%d" % d, _shares(n, r=3, stop=stop), stop_at=stop)


# ---- L: k_seq -----------------------------------------------------------------------------------------------------------

def l_cap(seed, d, slack=2, k=4.0, filt=False):
    """cap(d) - slack rows, three quarters of them pcores.  With C = min(64, 512 / d) points staged at a time, creations on the
    last point of the first chunk and the first of the second (slack 2; with slack 1 only the first), and the one that finds the
    image full on the first point of the third chunk (slack 1: of the second): k_seq takes exactly the points before it.  slack 0:
    k_seq_g from the first point.  Around them joins, a promotion, ties between pcore rows q and q + 64 (one lane of k_seq) and
    between the first and the last row; behind the stop the same on k_seq_g (or the windows)."""
    cap, C = seq_cap_rows(d), seq_chunk(d)
    m = cap - slack
    m_p = (3 * m) // 4
    m_o = m - m_p
    D = _Design(seed, d, k=k, filt=filt)
    D.fill(m_p, m_o, promotable=(0, 1, m_o - 2, m_o - 1))  # (1, m_o - 2: the tied pair - promoted out of the tie)
    p, o = D.rows["p"], D.rows["o"]
    t1 = D.place([p[0], p[m_p - 1]], [D.axis(0, -TIE), D.axis(0, TIE)])
    t2 = D.place([p[65], p[1]], [D.axis(1, -TIE), D.axis(1, TIE)]) if m_p >= 70 else None
    t3 = D.place([p[2], p[m_p - 2]], [D.axis(0, TIE), D.axis(1, TIE)])
    t4 = D.place([o[1], o[m_o - 2]], [D.axis(1, -TIE), D.axis(1, TIE)]) if m_o >= 5 else None
    D.seal()
    creations = {2: [C - 1, C, 2 * C], 1: [C - 1, C], 0: [0]}[slack]
    stop = creations[-1]
    n = 3 * C + 1
    free_p = [r for r in p[3:m_p - 2] if r.idx != 65]
    made = []
    while D.at < n:
        i = D.at
        if i in creations or i == n - 2:
            made.append(D.create())
        elif i == 1:
            D.tie(t1, [p[0], p[m_p - 1]])
        elif i == 2 and C > 4:
            D.promote(o[0])
        elif i == 3 and t2 is not None:
            D.tie(t2, [p[65], p[1]])
        elif i == stop + 1:
            D.tie(t3, [p[2], p[m_p - 2]])
        elif i == stop + 2:
            D.promote(o[m_o - 1])
        elif i == stop + 3 and t4 is not None:
            D.tie(t4, [o[1], o[m_o - 2]])
        elif i == stop + 4 and made:
            D.join(made[-1])
        elif i % 5 == 4 and m_o >= 6:
            D.join(o[2 + (i // 5) % (m_o - 4)])
        else:
            D.join(free_p[i % len(free_p)])
    name = {2: "l-cap-d%d", 1: "l-cap-1-d%d", 0: "l-cap-0-d%d"}[slack] % d
    return D.case(name, _shares(n, stop=stop, r_possible=False), stop_at=stop, cap=cap, chunk=C)


def l_n(seed, d, n):
    """n points (1, C - 1, C, C + 1 by the cases) on 40 rows - 17 where the image holds 25: the table must fit with the call's
    creations -, a creation on the last point."""
    cap = seq_cap_rows(d)
    m = min(40, cap - 8)
    D = _Design(seed, d)
    D.fill(m - m // 4, m // 4, promotable=(0,))
    D.seal()
    p, o = D.rows["p"], D.rows["o"]
    made = None
    while D.at < n:
        i = D.at
        if i == n - 1 or i == 2:
            made = D.create()
        elif i == 1:
            D.promote(o[0])
        elif i == 4:
            D.join(made)
        elif i % 3 == 0:
            D.join(o[1 + i % (len(o) - 1)])
        else:
            D.join(p[i % len(p)])
    return D.case("l-n%d-d%d" % (n, d), _shares(n, r_possible=False))


# ---- G: k_seq_g ---------------------------------------------------------------------------------------------------------

def g_dims(seed, d, filt=False, k=4.0):
    """100 + 64 rows beyond the LDS kernels' reach, 3 chunks + 1 points (never fewer than the lattice generator plants, and never
    fewer than the events below).  Without filter: table_util.lattice as it stands - copies of one row at list positions 0, 31, 32,
    33 and the last (equal distances), radii exactly on eps^2 and beyond it.  With the filter (and k = 3): ties in both lists, a
    promotion, a tie with the promoted row, creations and joins of the created rows."""
    n = 3 * seq_g_chunk(d) + 1
    if not filt:
        pcores, outliers, par, X, meta = T.lattice(seed, 100, 64, d, n)
        meta = dict(meta, kind="seq-edge", base="lattice", name="g-dims-d%d" % d, events=[], ties=[], uid=None, path=None,
                    shares=_shares(len(X), g=len(X), r_possible=False))
        if d > WINDOW_MAX_DIM:
            del meta["shares"]["seq2-seqg0"]
        return pcores, outliers, par, X, meta
    D = _Design(seed, d, k=k, filt=True)
    D.fill(100, 64, promotable=(0, 31, 32, 63))            # (31, 32: the tied pair - promoted out of the tie)
    p, o = D.rows["p"], D.rows["o"]
    t1 = D.place([p[0], p[99]], [D.axis(0, -TIE), D.axis(0, TIE)])
    c = D.place([p[63], p[64], o[0]], [D.axis(0, 2 * TIE), D.axis(1, 2 * TIE), 0.0])
    t2 = D.place([o[31], o[32]], [D.axis(1, -TIE), D.axis(1, TIE)])
    D.seal()
    D.tie(t1, [p[0], p[99]])
    a = D.create()
    D.tie(c, [p[63], p[64]], absorbed=False, then=o[0])
    D.tie(c + D.axis(0, TIE), [p[63], o[0]])
    D.join(a)
    D.tie(t2, [o[31], o[32]])
    D.tie(c + D.axis(1, TIE), [p[64], o[0]])
    D.promote(o[63])
    D.create()
    D.join(p[50])
    while D.at < n:
        D.join(p[1 + D.at % 60] if D.at % 2 else o[1 + D.at % 29])
    m = D.at
    sh = _shares(m, g=m, r_possible=False)
    del sh["seq2-seqg0"]
    return D.case("g-dims-filter-d%d" % d, sh)


def g_stride(seed, d, n=300):
    """1 025 pcores and 1 025 outliers: thread 0 of k_seq_g holds rows 0 and 1 024 of each list.  Row 1 024 of each list sits on c,
    row 0 1/4 from it along axis 0, row 1 023 along axis 1: points tied between 0 / 1 024 (one thread) and 1 023 / 1 024 (last and
    first thread, last and first wave); rows 63 / 64 around a point of their own (two waves).  An outlier 1/4 beside pcore row
    500 is promoted (the point on it is refused by row 500), the next point is tied between the two."""
    m = 1025
    D = _Design(seed, d)
    D.fill(m, m, promotable=(7, 500))
    p, o = D.rows["p"], D.rows["o"]
    cs = {}
    for kind, rows in (("p", p), ("o", o)):
        cs[kind] = D.place([rows[1024], rows[0], rows[1023]], [0.0, D.axis(0, 2 * TIE), D.axis(1, 2 * TIE)])
        cs[kind + "w"] = D.place([rows[63], rows[64]], [D.axis(0, -TIE), D.axis(0, TIE)])
    cp = D.place([p[500], o[500]], [0.0, D.axis(0, 2 * TIE)])
    D.seal()
    script = [
        lambda: D.tie(cs["p"] + D.axis(0, TIE), [p[0], p[1024]]),
        lambda: D.tie(cs["o"] + D.axis(0, TIE), [o[0], o[1024]]),
        lambda: D.create(),
        lambda: D.tie(cs["p"] + D.axis(1, TIE), [p[1023], p[1024]]),
        lambda: D.tie(cs["o"] + D.axis(1, TIE), [o[1023], o[1024]]),
        lambda: D.tie(cs["pw"], [p[63], p[64]]),
        lambda: D.tie(cs["ow"], [o[63], o[64]]),
        lambda: D.promote(o[500]),
        lambda: D.tie(cp + D.axis(0, TIE), [p[500], o[500]]),
        lambda: D.promote(o[7]),
        lambda: D.join(o[7]),
    ]
    for i, step in enumerate(script):
        step()
        D.join(p[100 + i])
    made = []
    while D.at < n:
        i = D.at
        if i % 37 == 0:
            made.append(D.create())
        elif i % 37 == 5 and made:
            D.join(made[-1])
        elif i % 2:
            D.join(o[100 + (i * 7) % 390])
        else:
            D.join(p[100 + (i * 11) % 390])
    sh = _shares(n, g=n, r_possible=False)
    if d > WINDOW_MAX_DIM:
        del sh["seq2-seqg0"]
    return D.case("g-stride-d%d" % d, sh)


def g_one_point(seed, d, n):
    """1 024 dimensions, one point per chunk: n = 1 a point tied between pcore rows 0 and 149, n = 2 a promotion first."""
    D = _Design(seed, d)
    D.fill(150, 50, promotable=(49,))
    p, o = D.rows["p"], D.rows["o"]
    t = D.place([p[149], p[0]], [D.axis(0, -TIE), D.axis(0, TIE)])
    D.seal()
    if n == 2:
        D.promote(o[49])
    D.tie(t, [p[149], p[0]])
    sh = _shares(n, g=n, r_possible=False)
    del sh["seq2-seqg0"]
    return D.case("g-one-point-d%d-n%d" % (d, n), sh)


SEQ_EDGE_CASES = {}
for _d in (2, 3, 4):
    SEQ_EDGE_CASES["r-lanes16-d%d" % _d] = (r_lanes16, dict(seed=1100 + _d, d=_d))
for _at in (0, 63, 64, 100):
    SEQ_EDGE_CASES["r-p63-at%d-d3" % _at] = (r_p63, dict(seed=1110 + _at, d=3, at=_at))
SEQ_EDGE_CASES["r-p63-at63-d2"] = (r_p63, dict(seed=1121, d=2, at=63))
SEQ_EDGE_CASES["r-p63-at63-d4"] = (r_p63, dict(seed=1122, d=4, at=63))
SEQ_EDGE_CASES["r-p64-d3"] = (r_p63, dict(seed=1123, d=3, m_p=64))
SEQ_EDGE_CASES["r-p65-d3"] = (r_p63, dict(seed=1124, d=3, m_p=65))
SEQ_EDGE_CASES["r-o-fill-d3"] = (r_o_fill, dict(seed=1125, d=3))
SEQ_EDGE_CASES["r-o-fill-d4"] = (r_o_fill, dict(seed=1126, d=4))
SEQ_EDGE_CASES["r-o-full-d2"] = (r_o_full, dict(seed=1127, d=2, m_o=256))
SEQ_EDGE_CASES["r-o-over-d4"] = (r_o_full, dict(seed=1128, d=4, m_o=193))
SEQ_EDGE_CASES["r-slot-ties-d3"] = (r_slot_ties, dict(seed=1129, d=3))
SEQ_EDGE_CASES["r-reload-d3"] = (r_reload, dict(seed=1130, d=3))
SEQ_EDGE_CASES["r-l-g-d4"] = (r_l_g, dict(seed=1131, d=4))
# every <FILTER, POW2> instance of k_seq meets a cap: d = 5, 40, 64 plain, 8 with the filter, 13 with k = 3, 20 with both
L_CAP_VARIANT = {5: {}, 8: dict(filt=True), 13: dict(k=3.0), 20: dict(filt=True, k=3.0), 40: {}, 64: {}}
for _d, _kw in L_CAP_VARIANT.items():
    SEQ_EDGE_CASES["l-cap-d%d" % _d] = (l_cap, dict(seed=1200 + _d, d=_d, **_kw))
SEQ_EDGE_CASES["l-cap-1-d20"] = (l_cap, dict(seed=1271, d=20, slack=1))
SEQ_EDGE_CASES["l-cap-0-d20"] = (l_cap, dict(seed=1272, d=20, slack=0))
L_N = {_d: (1, seq_chunk(_d) - 1, seq_chunk(_d), seq_chunk(_d) + 1) for _d in (8, 20, 64)}
for _d, _ns in L_N.items():
    for _n in _ns:
        SEQ_EDGE_CASES["l-n%d-d%d" % (_n, _d)] = (l_n, dict(seed=1300 + _d, d=_d, n=_n))
G_DIMS = (65, 127, 128, 129, 191, 192, 193, 512, 513, 1024)
for _d in G_DIMS:
    SEQ_EDGE_CASES["g-dims-d%d" % _d] = (g_dims, dict(seed=1400 + _d, d=_d))
for _d in (128, 513):
    SEQ_EDGE_CASES["g-dims-filter-d%d" % _d] = (g_dims, dict(seed=2500 + _d, d=_d, filt=True, k=3.0))
SEQ_EDGE_CASES["g-stride-d20"] = (g_stride, dict(seed=1520, d=20))
SEQ_EDGE_CASES["g-stride-d129"] = (g_stride, dict(seed=1529, d=129))
for _n in (1, 2):
    SEQ_EDGE_CASES["g-one-point-d1024-n%d" % _n] = (g_one_point, dict(seed=1600 + _n, d=1024, n=_n))
del _d, _at, _kw, _ns, _n


def build_seq_edge(name):
    gen, kw = SEQ_EDGE_CASES[name]
    case = gen(**kw)
    assert case[4]["kind"] == "seq-edge" and case[4]["name"] == name, (name, case[4]["name"])
    return case


def modes_of(case):
    """The forced modes a case runs in: sequential=2 always, without k_seq_r where it could run (d <= 4), without k_seq_g where
    the table outgrows k_seq's image (the windows then take points)."""
    sh = case[4]["shares"]
    return [m for m in MODES if m in sh and (m != "seq2-seqg0" or sh[m]["window_points"] > 0)]


# ---- the design, held against the oracle's result -------------------------------------------------------------------------

def _dist(x, cen, pref):
    return ((x - cen) ** 2 / pref).sum(axis=-1)


def ties_hold(case):
    """Per designed tie: the distances of its rows to its point, recomputed in numpy from the injected centroids and entries
    (rows of a tie are untouched until their point, a promotion leaves both where they are) - equal bit for bit, and smaller than
    the distance of every other injected row of the tied rows' list.  Returns the number of ties."""
    pcores, outliers, par, X, meta = case
    by_uid = {}
    for t in (pcores, outliers):
        if t is not None:
            for r in range(len(t)):
                by_uid[int(t.uid[r])] = (t, r)
    for tie in meta["ties"]:
        x = X[tie["at"]]
        dist = []
        for uid, cen in tie["rows"]:
            t, r = by_uid[uid]
            assert np.array_equal(t.cen[r], cen)
            dist.append(_dist(x, t.cen[r], t.pref[r]))
        assert len(dist) >= 2 and all(a == dist[0] for a in dist), (meta["name"], tie["at"], dist)
        tied = {uid for uid, _ in tie["rows"]}
        own = pcores if tie["stage"] == "p" else outliers     # (a promoted row of a pcore tie is looked up in the outliers above)
        others = np.array([int(u) not in tied for u in own.uid])
        if others.any():
            assert _dist(x, own.cen[others], own.pref[others]).min() > dist[0], (meta["name"], tie["at"])
    return len(meta["ties"])


def check_seq_edge(case, res):
    """Asserts on the ORACLE's result that a case holds its design (no GPU involved): uid and path of every point, every designed
    promotion and creation at its index with the list sizes before and after as the paths imply them, the ties bit-equal and won
    by the smallest key, the sizes of both lists at the end."""
    pcores, outliers, par, X, meta = case
    uid, path = res["uid"], res["path"]
    if meta.get("base") == "lattice":
        T.check_online((pcores, outliers, par, X, dict(meta, kind="lattice")), res)
        tag = meta["tag"]
        assert (path[tag == "equal"] == 0).all() and (tag == "equal").sum() == 4
        assert sorted(uid[tag == "equal"]) == sorted(pcores.uid[meta["eq_at"]])
        assert (path[tag == "beyond"] == 2).all() and (tag == "beyond").sum() == 4
        e1 = np.zeros(X.shape[1])
        e1[1] = 0.5
        for x in X[tag == "equal"]:                                     # radius exactly ON eps^2, accepted
            row = [p for p in meta["eq_at"] if np.array_equal(pcores.cen[p], x - e1)]
            assert len(row) == 1 and T.tentative(pcores, np.array(row), x[None, :], par)[1][0] == par.eps_sq
        assert (tag == "copy_p").sum() == 5 and (tag == "copy_o").sum() == 5
        for t, name in ((pcores, "copy_p"), (outliers, "copy_o")):      # five coincident rows: five equal distances
            x = X[np.flatnonzero(tag == name)[0]]
            dist = _dist(x, t.cen, t.pref)
            assert (dist == dist.min()).sum() == 5 and dist.min() == 0.0
        return
    name = meta["name"]
    bad = np.flatnonzero((uid != meta["uid"]) | (path != meta["path"]))
    assert len(bad) == 0, "%s: point %d is (uid %d, path %d), designed (uid %d, path %d); %d points differ" % (
        name, bad[0], uid[bad[0]], path[bad[0]], meta["uid"][bad[0]], meta["path"][bad[0]], len(bad))
    n_p = len(pcores) if pcores is not None else 0
    n_o = len(outliers) if outliers is not None else 0
    events = {e["at"]: e for e in meta["events"]}
    assert len(events) == len(meta["events"])
    for i, code in enumerate(path):
        if code in (2, 5):
            e = events.pop(i, None)
            assert e is not None, "%s: point %d has path %d, no event was designed there" % (name, i, code)
            assert e["what"] == ("creation" if code == 2 else "promotion") and e["uid"] == uid[i], (name, e)
            after = (n_p + (code == 5), n_o + (1 if code == 2 else -1))
            assert e["n_p"] == (n_p, after[0]) and e["n_o"] == (n_o, after[1]), (name, e, n_p, n_o)
            n_p, n_o = after
    assert not events, "%s: designed events that did not happen: %r" % (name, sorted(events))
    o = res["o"]
    assert (len(o.table(0)["uid"]), len(o.table(1)["uid"])) == (n_p, n_o)
    ties_hold(case)
    for tie in meta["ties"]:
        i = tie["at"]
        if tie["absorbed"]:
            assert uid[i] == tie["winner"], "%s: tied point %d went to %d, the smallest key is %d" % (name, i, uid[i], tie["winner"])
        else:
            assert uid[i] not in {u for u, _ in tie["rows"]}, (name, tie)
