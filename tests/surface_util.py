"""The goldens of tests/golden/surface/: what the Python reference computes at the places the fuzz tests and the
injected-table referees were designed to hit (tests/golden/make_golden_surface.py records them; test_reference_surface_cpu.py
holds the oracle against them, test_reference_surface.py the kernels).

One RECORD is what either side leaves behind after one call: per-point labels, both microcluster lists, the id counters, the
derived parameters, the clusters of the offline phase.  Integer columns, weights and parameters are kept in full; the wide
float columns (cf1, cf2, cen, pref of the lists and of the clusters) as the SHA-256 of their bytes - a differing digest names
the case, the call and the column, and the GPU-versus-oracle tests of the same case then find the element.  `make_record`
builds a record from any side's results, `same_record` compares two of them bit for bit (bytes, not values: -0.0 is not 0.0
and a NaN is equal to itself only with the same payload).

A file holds the records of many cases in four pooled arrays (one per element type) plus one row of lengths per record:
thousands of small arrays as zip members of their own would cost more than their content.
"""
import hashlib
import json
import os

import numpy as np

import table_util as T
from golden_util import GOLDEN

SURFACE = os.path.join(GOLDEN, "surface")
LARGEST_GOLDEN = os.path.join(GOLDEN, "blob_d20.npz")   # no file of the directory may be larger
DIR_LIMIT = 2_000_000                                    # nor the directory larger than this

FUZZ_MAX_POINTS = 4000        # test_fuzz_parity._case(seed): the seeds whose largest timepoint has at most so many points (all)
SEQ_R_MAX_POINTS = 3000       # test_sequential._seq_r_case(seed) alike
OFFLINE_MAX_PCORES = 700      # table_util.OFFLINE_TABLES
ONLINE_MAX_ROW_POINTS = 600_000   # table_util.ONLINE_TABLES: injected rows x points

LIST_COLS = ("id", "uid", "w", "cf1", "cf2", "cen", "pref")
DIGESTED = ("cf1", "cf2", "cen", "pref")

# (field, pool): i = int64, f = float64, c = int8, b = bytes (SHA-256 digests)
FIELDS = ([("params", "f"), ("xsha", "b"), ("labels_uid", "i"), ("labels_path", "c")]
          + [("%s_%s" % (kind, col), "b" if col in DIGESTED else "f" if col == "w" else "i")
             for kind in ("pcore", "outlier") for col in LIST_COLS]
          + [("cl_members", "i"), ("cl_offsets", "i"), ("cl_w", "f")] + [("cl_" + col, "b") for col in DIGESTED]
          + [("off_core", "c"), ("off_pdim", "i"), ("off_nn", "i"), ("off_nw", "i"), ("mid_pref", "f")])
POOLS = {"i": np.int64, "f": np.float64, "c": np.int8, "b": np.uint8}

LISTS = [f for f, _ in FIELDS if f.startswith(("pcore_", "outlier_"))]
CLUSTERS = [f for f, _ in FIELDS if f.startswith("cl_")]
OFFLINE_INFO = ["off_core", "off_pdim", "off_nn", "off_nw"]


def sha(a):
    """SHA-256 of a float column's bytes (float64, C order) as 32 uint8."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest(), dtype=np.uint8)


def make_record(params=None, X=None, uid=None, path=None, tables=None, clusters=None, info=None, mid_pref=None):
    """A record from one side's results.  params: (pi, mu, omicron, pcore_last_id, outlier_last_id); tables: the pcore and the
    outlier list as dicts of id, uid, w, cf1, cf2, cen, pref; clusters: dicts of members (merge order), w, cf1, cf2, cen,
    pref; info: core, pdim, nn, nw per pcore position.  What a side does not have stays out of the record."""
    r = {}
    if params is not None:
        r["params"] = np.array([float(x) for x in params], dtype=np.float64)
    if X is not None:
        r["xsha"] = sha(X)
    if uid is not None:
        r["labels_uid"] = np.asarray(uid, dtype=np.int64)
    if path is not None:
        r["labels_path"] = np.asarray(path, dtype=np.int8)
    if tables is not None:
        for kind, tab in zip(("pcore", "outlier"), tables):
            for col in LIST_COLS:
                a = tab[col]
                r["%s_%s" % (kind, col)] = (sha(a) if col in DIGESTED else np.asarray(a, dtype=np.float64) if col == "w"
                                            else np.asarray(a, dtype=np.int64))
    if clusters is not None:
        r["cl_members"] = np.array([int(x) for c in clusters for x in c["members"]], dtype=np.int64)
        r["cl_offsets"] = np.cumsum([0] + [len(c["members"]) for c in clusters]).astype(np.int64)
        r["cl_w"] = np.array([float(c["w"]) for c in clusters], dtype=np.float64)
        for col in DIGESTED:
            r["cl_" + col] = sha(np.array([np.asarray(c[col], dtype=np.float64) for c in clusters], dtype=np.float64))
    if info is not None:
        r["off_core"] = np.asarray(info["core"], dtype=np.int8)
        for key in ("pdim", "nn", "nw"):
            r["off_" + key] = np.asarray(info[key], dtype=np.int64)
    if mid_pref is not None:
        r["mid_pref"] = np.ascontiguousarray(mid_pref, dtype=np.float64).reshape(-1)
    return r


def same_record(got, exp, fields, what):
    """Bit equality of `fields` between a side's record and the golden one; the message names case, call and column."""
    for f in fields:
        assert f in got and f in exp, "%s: %s missing (%s)" % (what, f, "golden" if f in got else "this side")
        a, b = got[f], exp[f]
        if a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes():
            continue
        if dict(FIELDS)[f] == "b":
            raise AssertionError("%s: column %s differs from the reference's (SHA-256 of its bytes)" % (what, f))
        if a.shape != b.shape:
            raise AssertionError("%s: %s has %r entries, the reference's %r" % (what, f, a.shape, b.shape))
        assert a.dtype == b.dtype, "%s: %s is %s, the reference's %s" % (what, f, a.dtype, b.dtype)
        bits = {1: np.uint8, 8: np.uint64}[a.dtype.itemsize]
        at = int(np.flatnonzero(a.view(bits) != b.view(bits))[0])
        raise AssertionError("%s: %s differs from the reference's, first at %d: %r / %r" % (what, f, at, a[at], b[at]))


def clusters_of(rec):
    """[dict(members=...)] of a record, for the structure checks."""
    off = rec["cl_offsets"]
    return [dict(members=rec["cl_members"][off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def info_of(rec):
    info = dict(core=rec["off_core"], pdim=rec["off_pdim"].astype(np.int32), nn=rec["off_nn"].astype(np.int32),
                nw=rec["off_nw"].astype(np.int32))
    info["num_core"] = int(info["core"].sum())
    return info


def table_of(rec, kind):
    return {col: rec["%s_%s" % (kind, col)] for col in ("id", "uid", "w")}


# ---- files ------------------------------------------------------------------------------------------------------------

def save_pack(path, records, meta=None):
    """records: [(name, record)] in the order they are to be kept."""
    pools = {p: [] for p in POOLS}
    lens = np.full((len(records), len(FIELDS)), -1, dtype=np.int32)
    for i, (_, rec) in enumerate(records):
        assert set(rec) <= set(f for f, _ in FIELDS), sorted(set(rec) - set(f for f, _ in FIELDS))
        for j, (f, p) in enumerate(FIELDS):
            if f in rec:
                a = np.ascontiguousarray(rec[f], dtype=POOLS[p]).reshape(-1)
                lens[i, j] = len(a)
                pools[p].append(a)
    out = {"pool_" + p: np.concatenate(pools[p]) if pools[p] else np.zeros(0, POOLS[p]) for p in POOLS}
    head = dict(names=[n for n, _ in records], fields=[f for f, _ in FIELDS], meta=meta or {})
    out["head"] = np.frombuffer(json.dumps(head, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(path, lens=lens, **out)


class Pack(object):
    """The records of one file by name."""

    def __init__(self, path):
        z = np.load(path, allow_pickle=False)
        head = json.loads(z["head"].tobytes().decode())
        assert head["fields"] == [f for f, _ in FIELDS], "%s was written with another field list: regenerate" % path
        self.names, self.meta = head["names"], head["meta"]
        lens = z["lens"]
        pools = {p: z["pool_" + p] for p in POOLS}
        at = {p: 0 for p in POOLS}
        self.records = {}
        for i, name in enumerate(self.names):
            rec = {}
            for j, (f, p) in enumerate(FIELDS):
                n = int(lens[i, j])
                if n >= 0:
                    rec[f] = pools[p][at[p]:at[p] + n]
                    at[p] += n
            self.records[name] = rec
        assert all(at[p] == len(pools[p]) for p in POOLS)


_packs = {}


def load_set(prefix, directory=SURFACE):
    """(records by name, names in order, metas) of every file `prefix`*.npz of the directory."""
    key = (prefix, directory)
    if key not in _packs:
        records, names, metas = {}, [], []
        for fn in sorted(os.listdir(directory)) if os.path.isdir(directory) else []:
            if fn.startswith(prefix) and fn.endswith(".npz"):
                p = Pack(os.path.join(directory, fn))
                records.update(p.records)
                names += p.names
                metas.append(p.meta)
        _packs[key] = (records, names, metas)
    return _packs[key]


def cases_of(prefix):
    """The case names of a set, in order (a record's name is `case@call`)."""
    seen = []
    for n in load_set(prefix)[1]:
        c = n.rsplit("@", 1)[0]
        if c not in seen:
            seen.append(c)
    return seen


def stream_dims():
    """case -> dimensions of every recorded stream (kept in the files, so that nobody builds a stream to learn its width)."""
    out = {}
    for meta in load_set("streams_")[2]:
        out.update(meta.get("dims", {}))
    return out


def calls_of(prefix, case):
    """The golden records of a case in call order."""
    records = load_set(prefix)[0]
    out = []
    while "%s@%d" % (case, len(out)) in records:
        out.append(records["%s@%d" % (case, len(out))])
    assert out, "no golden record of %s" % case
    return out


# ---- the cases: inputs regenerated from their seeds ---------------------------------------------------------------------

def stream_case(case):
    """(config, timepoints) of `fuzz-<seed>` / `seqr-<seed>`."""
    kind, seed = case.split("-")
    if kind == "fuzz":
        from test_fuzz_parity import _case
        cfg, _, Xs = _case(int(seed))
    else:
        from test_sequential import _seq_r_case
        cfg, Xs = _seq_r_case(int(seed))
    return cfg, Xs


def stream_selection():
    """What the generator records: (fuzz seeds, fuzz seeds left out, seq_r seeds), by the size of the largest timepoint."""
    from test_fuzz_parity import _case
    from test_sequential import _seq_r_case
    big = {s: max(len(X) for X in _case(s)[2]) for s in range(192)}
    fuzz = [s for s in range(192) if big[s] <= FUZZ_MAX_POINTS]
    seqr = [s for s in range(96) if max(len(X) for X in _seq_r_case(s)[1]) <= SEQ_R_MAX_POINTS]
    return fuzz, [s for s in range(192) if s not in fuzz], seqr


def check_inputs(case, Xs, golden):
    for t, X in enumerate(Xs):
        assert golden[t]["xsha"].tobytes() == sha(X).tobytes(), \
            "%s timepoint %d: numpy Generator stream changed: regenerate the goldens" % (case, t)


def boundary_cases():
    """name -> (seed, m_p, m_o, d, all rows flagged): test_boundary_tables.SHAPES without the 50 000-row shape, and the cases
    of test_repeated_calls_empty_the_table."""
    from test_boundary_tables import SHAPES
    out = {}
    for m_p, m_o, d in SHAPES:
        if m_p + m_o < 50_000:
            out["boundary-%d+%dx%d" % (m_p, m_o, d)] = (1000 * d + m_p, m_p, m_o, d, False)
    for m_p, m_o, d in [(7, 0, 4), (64, 33, 24), (300, 300, 16)]:
        out["flagged-%d+%dx%d" % (m_p, m_o, d)] = (77 + d, m_p, m_o, d, True)
    return out


def boundary_case(name):
    """(pcores, outliers or None, params) as the two tests of test_boundary_tables build them."""
    from test_boundary_tables import boundary_lists
    seed, m_p, m_o, d, flagged = boundary_cases()[name]
    pcores, outliers, par = boundary_lists(seed, m_p, m_o, d)
    if flagged:
        pcores = T.Table(pcores.cen, 1e-5, pcores.pref, np.full(m_p, 0.3), pcores.id, pcores.uid)
        outliers = T.Table(outliers.cen, 1e-5, outliers.pref, np.full(m_o, 0.2), outliers.id, outliers.uid)
        if not m_o:
            outliers = None
    return pcores, outliers, par


def offline_cases():
    return [n for n, (_, kw) in T.OFFLINE_TABLES.items() if kw["mp"] <= OFFLINE_MAX_PCORES]


def online_cases():
    """The ONLINE_TABLES with injected rows x points within the limit (the set_params cases inject nothing)."""
    out = []
    for name, (gen, kw) in T.ONLINE_TABLES.items():
        if gen is T.victims:
            rows = kw["pairs"] * (3 if kw.get("filt") else 2) + (max(1, kw["pairs"] // 8) if kw.get("on_outliers") else 0)
            points = kw.get("points") or kw["pairs"]
        elif gen is T.victims_by_set_params:
            rows, points = 0, kw["pairs"]
        else:
            rows, points = kw["m_p"] + kw["m_o"], kw["n"]
        if rows * points <= ONLINE_MAX_ROW_POINTS:
            out.append(name)
    return out
