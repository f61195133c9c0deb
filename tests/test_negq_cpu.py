"""The logicle width estimated from the events, without a GPU: the rule on known values, the host route
(_lib.negative_quantiles_host, fcs.estimate_logicle(handle=None)) against the referee of negq_util bit for bit on FCS files
written by fcs_util, the sidecar's "estimate" and "q", the refusals, and the designed key sets of the GPU test checked for the
property each claims."""
import json
import os

import numpy as np
import pytest

import fcs_util as F
import negq_util as N
import transform_util as U

T0, M0 = 262144.0, 4.5
MARKERS = ["CD3", "CD4", "CD8"]
NAMES = ["Time", "CD4", "FSC-A", "CD3", "CD8"]
COMP = ["CD3", "FSC-A", "CD4"]


def test_logicle_w_on_known_values():
    from chronoclust_amd import fcs
    for r, W in ((-50.0, 0.39021504119217854), (-300.0, 0.7792906663840005), (-1.0, 0.0), (-1e7, 2.25)):
        got = fcs.logicle_w(1, r, r, 0.0, T0, M0)
        assert got == W and isinstance(got, float), (r, got)
        assert got == N.width(1, r, T0, M0), r
    assert fcs.logicle_w(0, 0.0, 0.0, 0.0, T0, M0) == 0.0
    with pytest.raises(ValueError):
        fcs.logicle_w(3, -np.inf, -np.inf, 0.0, T0, M0)
    # the interpolation is numpy's own
    assert fcs.logicle_w(4, -300.0, -50.0, 0.25, T0, M0) == N.width(4, np.quantile(np.array([-300.0, -50.0]), 0.25), T0, M0)


def write(tmp_path, name, kind, n, seed, pnr=65536, spill_seed=3):
    """One FCS file of n events: "f32" big-endian float32, "u16" little-endian uint16 - both on the device route - or
    "mixed": integers of differing $PnB, which read_fcs decodes on the host.  Every file carries a spillover of its own."""
    rng = np.random.default_rng(seed)
    spill = U.spillover(len(COMP), spill_seed)[0]
    extra = {"$SPILLOVER": U.spillover_text(COMP, spill)}
    path = os.path.join(str(tmp_path), name)
    if n == 0:
        # no event: the HEADER's DATA offsets and $BEGINDATA / $ENDDATA are 0, $TOT is 0
        blob = F.fcs_bytes(b"", len(NAMES), "F", N.BIG, 32, names=NAMES, tot=0, ranges=pnr,
                           extra=dict(extra, **{"$BEGINDATA": "0", "$ENDDATA": "0"}))
        with open(path, "wb") as f:
            f.write(blob[:26] + b"%8d" % 0 + blob[34:])
    elif kind == "f32":
        rec = rng.normal(30.0, 200.0, (n, len(NAMES))).astype(np.float32)
        F.write_fcs(path, F.fast_records(rec, N.BIG), len(NAMES), "F", N.BIG, 32, names=NAMES, tot=n, ranges=pnr, extra=extra)
    elif kind == "u16":
        rec = rng.integers(0, 4096, (n, len(NAMES)), dtype=np.uint16)
        F.write_fcs(path, F.fast_records(rec, N.LITTLE), len(NAMES), "I", N.LITTLE, 16, names=NAMES, tot=n, ranges=pnr, extra=extra)
    else:
        widths = [4, 2, 2, 4, 2]
        rec = rng.integers(0, 4096, (n, len(NAMES))).tolist()
        F.write_fcs(path, F.records(rec, "u", widths, N.LITTLE), len(NAMES), "I", N.LITTLE, [8 * w for w in widths], names=NAMES, tot=n,
                    ranges=pnr, extra=extra)
    return path


def sources_of(paths, compensate=True):
    """The files as ListModes with their compensation, the host-decoded layout as native float64 records: read through
    read_fcs, which the suite holds to fcs_util elsewhere."""
    from chronoclust_amd import _lib, fcs
    out = []
    for p in paths:
        pts = fcs.read_fcs(p, columns=MARKERS, compensate=compensate)[0]
        if not isinstance(pts, _lib.ListMode):
            pts = _lib.ListMode(np.ascontiguousarray(pts), pts.shape[0], pts.shape[1], np.float64)
        out.append(pts)
    return out


POOLS = {"one file": [("f32", 130, 1)], "two files": [("f32", 130, 1), ("u16", 200, 2)],
         "three with an empty one": [("u16", 65, 4), ("f32", 0, 5), ("mixed", 90, 6)],
         "the host layout alone": [("mixed", 130, 7)]}


@pytest.mark.parametrize("pool", sorted(POOLS))
def test_the_host_route_against_the_referee(tmp_path, pool):
    from chronoclust_amd import _lib, fcs
    paths = [write(tmp_path, "f%d.fcs" % i, kind, n, seed, spill_seed=seed) for i, (kind, n, seed) in enumerate(POOLS[pool])]
    src = sources_of(paths)
    assert any(s.n for s in src)
    for q in N.QS:
        exp = N.referee(src, q)
        assert (exp[0][:2] > 0).all(), "no negative value after the compensation: nothing is compared"  # (CD8 is not compensated)
        N.same(_lib.negative_quantiles_host(src, q), exp, "%s q=%g" % (pool, q))
        want = np.array([True, False, True])
        N.same(_lib.negative_quantiles_host(src, q, want), N.referee(src, q, want), "%s q=%g, two wanted" % (pool, q))
        rows = fcs.estimate_logicle(paths, columns=MARKERS, compensate=True, logicle={"W": "estimate", "M": 4.0}, q=q)
        assert list(rows) == MARKERS
        for c, name in enumerate(MARKERS):
            W = N.width(exp[0][c], exp[4][c], 65536.0, 4.0)
            assert rows[name] == {"T": 65536.0, "W": W, "M": 4.0, "A": 0.0}, (pool, q, name, rows[name], W)
    # cofactors and logicle rows of a source's transform are ignored
    dressed = [_lib.ListMode(s.buffer, s.n, s.src_cols, s.dtype, columns=s.columns, masks=s.masks,
                             transform=_lib.ListTransform(s.transform.comp_cols if s.transform else None,
                                                          s.transform.comp if s.transform else None, [5.0, 0.0, 0.0],
                                                          [[0.0] * 4, [0.0] * 4, [T0, 0.5, M0, 0.0]])) for s in src]
    N.same(_lib.negative_quantiles_host(dressed, 0.05), N.referee(src, 0.05), pool + ", dressed")


def test_rows_by_name_numeric_rows_and_a_q_of_their_own(tmp_path):
    from chronoclust_amd import fcs
    paths = [write(tmp_path, "a.fcs", "f32", 200, 11), write(tmp_path, "b.fcs", "f32", 90, 12)]
    src = sources_of(paths, compensate=False)
    spec = {"CD3": {"W": "estimate"}, "CD8": {"W": "estimate", "q": 0.25, "T": 5000, "M": 4}, "CD4": {"W": 0.75}}
    rows = fcs.estimate_logicle(paths, columns=MARKERS, logicle=spec)
    a, b = N.referee(src, 0.05), N.referee(src, 0.25)
    assert rows == {"CD3": {"T": 65536.0, "W": N.width(a[0][0], a[4][0], 65536.0, 4.5), "M": 4.5, "A": 0.0},
                    "CD4": {"T": 65536.0, "W": 0.75, "M": 4.5, "A": 0.0},
                    "CD8": {"T": 5000.0, "W": N.width(b[0][2], b[4][2], 5000.0, 4.0), "M": 4.0, "A": 0.0}}
    assert 0 < rows["CD3"]["W"] < 2.25 and 0 < rows["CD8"]["W"] < 2.0
    # the resolved rows are what read_fcs takes
    lm = fcs.read_fcs(paths[0], columns=MARKERS, logicle=rows)[0]
    assert lm._logicle.tolist() == [[rows[k][key] for key in "TWMA"] for k in MARKERS]
    # no negative value at all: W = 0
    c = write(tmp_path, "c.fcs", "u16", 70, 13)
    assert fcs.estimate_logicle([c], columns=["CD8"], logicle={"W": "estimate"})["CD8"]["W"] == 0.0


def test_sidecar_parsing_of_estimate_and_q(tmp_path):
    from chronoclust_amd import fcs
    path = write(tmp_path, "t.fcs", "f32", 10, 1)

    def sidecar(spec):
        with open(path + ".transform", "w") as f:
            json.dump(spec, f)
        return fcs.sidecar_transform(path)

    for logicle in ({"W": "estimate"}, {"W": "estimate", "q": 0.1, "M": 4}, {"CD3": {"W": "estimate", "q": 0.5}, "CD4": {"W": 1}}):
        assert sidecar({"compensate": True, "logicle": logicle}) == dict(compensate=True, cofactor=None, logicle=logicle)
    for bad in ({"W": "guess"}, {"W": 0.5, "q": 0.1}, {"q": 0.1}, {"W": "estimate", "q": "0.1"}, {"T": "estimate"},
                {"W": "estimate", "q": True}):
        with pytest.raises(ValueError, match="expected"):
            sidecar({"logicle": bad})
    assert fcs._is_logicle_row({"T": 1, "W": 0.5, "M": 4.5, "A": 0}) and fcs._is_logicle_row({"W": "estimate", "q": 0.05})


def test_the_value_errors(tmp_path):
    from chronoclust_amd import fcs
    a = write(tmp_path, "a.fcs", "f32", 50, 1)
    b = write(tmp_path, "b.fcs", "f32", 50, 2, pnr=20000)
    est = {"W": "estimate"}
    with pytest.raises(ValueError, match="estimate_logicle"):
        fcs.read_fcs(a, columns=MARKERS, logicle=est)
    with pytest.raises(ValueError, match="estimate_logicle"):
        fcs.read_fcs(a, columns=MARKERS, logicle={"CD4": est})
    with pytest.raises(ValueError, match="CD3.*T"):
        fcs.estimate_logicle([a, b], columns=MARKERS, logicle=est)  # ($PnR differs: two T for one channel)
    assert fcs.estimate_logicle([a, b], columns=MARKERS, logicle={"W": "estimate", "T": 9000})["CD3"]["T"] == 9000.0
    with pytest.raises(ValueError, match="CD19"):
        fcs.estimate_logicle([a], columns=MARKERS + ["CD19"], logicle=est)  # (a channel no file has)
    with pytest.raises(ValueError, match="CD19"):
        fcs.estimate_logicle([a], columns=MARKERS, logicle={"CD19": est})
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        fcs.estimate_logicle([a], columns=MARKERS, logicle=est, q=1.5)
    with pytest.raises(ValueError, match="logicle must be"):
        fcs.estimate_logicle([a], columns=MARKERS, logicle={"W": "guess"})
    # $PnE / $PnG as elsewhere
    rec = np.zeros((4, len(NAMES)), np.float32)
    for key, value in (("$P4G", "2"), ("$P5E", "4,1")):
        g = os.path.join(str(tmp_path), "g.fcs")
        F.write_fcs(g, F.fast_records(rec, N.BIG), len(NAMES), "F", N.BIG, 32, names=NAMES, tot=4, ranges=65536,
                    extra={key: value})
        with pytest.raises(ValueError, match=r"\%s" % key):
            fcs.estimate_logicle([g], columns=MARKERS, logicle=est)
    # -Inf among the negative values at the quantile: the channel is named
    rec = np.full((6, len(NAMES)), -np.inf, np.float32)
    i = os.path.join(str(tmp_path), "i.fcs")
    F.write_fcs(i, F.fast_records(rec, N.BIG), len(NAMES), "F", N.BIG, 32, names=NAMES, tot=6, ranges=65536)
    with pytest.raises(ValueError, match="CD3"):
        fcs.estimate_logicle([i], columns=MARKERS, logicle=est)
    # the host sibling's own refusals
    from chronoclust_amd import _lib
    src = sources_of([a])
    for q in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            _lib.negative_quantiles_host(src, q)
    with pytest.raises(ValueError):
        _lib.negative_quantiles_host([], 0.05)
    with pytest.raises(ValueError):
        _lib.negative_quantiles_host(src + sources_of([a])[:1], 0.05, want=[True])


def test_estimate_sidecars_pools_the_files_that_ask(tmp_path):
    from chronoclust_amd import fcs
    paths = [write(tmp_path, "t%d.fcs" % t, "f32", 80 + t, 20 + t) for t in range(3)]
    other = os.path.join(str(tmp_path), "x.npy")
    for p in paths:
        with open(p + ".columns", "w") as f:
            f.write("\n".join(MARKERS) + "\n")
    assert fcs.estimate_sidecars(paths + [other]) == ({}, {})
    spec = {"compensate": True, "cofactor": {"CD4": 150}, "logicle": {"W": "estimate", "M": 4}}
    for p in paths[:2]:
        with open(p + ".transform", "w") as f:
            json.dump(spec, f)
    with open(paths[2] + ".transform", "w") as f:
        json.dump({"compensate": True, "logicle": {"W": 0.5}}, f)
    overrides, resolved = fcs.estimate_sidecars(paths + [other])
    exp = N.referee(sources_of(paths[:2]), 0.05)
    assert sorted(overrides) == paths[:2] and sorted(resolved) == ["CD3", "CD8"]  # (CD4 has a cofactor: no logicle scale)
    for c, name in ((0, "CD3"), (2, "CD8")):
        assert resolved[name] == {"T": 65536.0, "W": N.width(exp[0][c], exp[4][c], 65536.0, 4.0), "M": 4.0, "A": 0.0}
        assert overrides[paths[0]][name] == resolved[name] and overrides[paths[1]][name] == resolved[name]
    # read_timepoint with the override is read_fcs with the resolved rows; without it the sidecar is refused
    from chronoclust_amd.scaling.scaler import read_timepoint
    lm = read_timepoint(paths[0], overrides)
    assert lm._logicle[:, 1].tolist() == [resolved["CD3"]["W"], 0.0, resolved["CD8"]["W"]] and lm._cofactors.tolist() == [0.0, 150.0, 0.0]
    with pytest.raises(ValueError, match="estimate_logicle"):
        read_timepoint(paths[0])
    assert read_timepoint(paths[2], overrides)._logicle[:, 1].tolist() == [0.5] * 3


def test_the_designed_key_sets_have_the_property_each_claims():
    sets = N.designed()
    rec, names = N.designed_records()
    assert rec.shape[1] == len(sets) == 19 and (rec[:, names.index("cnt 0")] > 0).all()
    for c, name in enumerate(names):  # the column holds the set and nothing else that counts
        v = rec[:, c]
        assert np.array_equal(np.sort(v[v < 0]), np.sort(sets[name][sets[name] < 0])), name
        assert len(set(N.keys(v[v < 0]).tolist())) == len(set(v[v < 0].tolist())), name + ": keys and values are one to one"
        order = np.argsort(v[v < 0], kind="stable")
        assert (np.diff(N.keys(v[v < 0])[order].astype(np.float64)) >= 0).all(), name + ": the keys order as the values do"
    assert N.digits_that_differ(sets["lowest mantissa byte"]) == [7]
    assert set(N.digits_that_differ(sets["exponent only"])) <= {0, 1} and len(set(sets["exponent only"].tolist())) == 101
    assert np.all(np.frexp(sets["exponent only"])[0] == -0.5)
    for p in range(8):
        assert N.digits_that_differ(sets["digit %d" % p]) == [p] and len(set(sets["digit %d" % p].tolist())) == 48
    assert N.digits_that_differ(sets["all equal"]) == []
    tie = np.sort(sets["heavy ties"])
    j = {q: int(np.floor((tie.size - 1) * q)) for q in N.QS + (0.26,)}
    assert tie.size == 101 and tie[j[0.05]] == tie[j[0.05] + 1] == -5.0  # j and j + 1 inside one tie
    assert tie[j[0.25]] == -5.0 and tie[j[0.25] + 1] == -4.0 and j[0.25] == 25  # j on the last of a tie
    assert tie[j[0.26]] == -4.0 and tie[j[0.26] - 1] == -5.0 and tie[j[0.26] + 1] == -4.0  # j on the first of the next
    assert [int((sets["cnt %d" % k] < 0).sum()) for k in range(3)] == [0, 1, 2]
    sub = sets["negative subnormals"]
    assert (sub < 0).all() and (np.abs(sub) < np.finfo(np.float64).tiny).all() and len(set(sub.tolist())) == sub.size
    z = sets["zeros"]
    assert np.signbit(z[z == 0]).sum() == 2 and (~np.signbit(z[z == 0])).sum() == 2 and (z < 0).sum() == 2
    nan = sets["NaN"]
    assert np.isnan(nan).sum() == 4 and np.signbit(nan[np.isnan(nan)]).sum() == 2 and (nan < 0).sum() == 39
    inf = sets["-Inf"]
    assert (inf == -np.inf).sum() == 1 and np.sort(inf[inf < 0])[0] == -np.inf
    # the seams: one n on each side of every edge of the selection's partition
    for edge in (N.WAVE, N.NEGQ_THREADS, N.NEGQ_CHUNK, 2 * N.NEGQ_CHUNK):
        assert {edge - 1, edge, edge + 1} <= set(N.SEAM_NS)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "chronoclust_amd", "csrc", "cc_negq.h")).read()
    assert "#define CC_NEGQ_CHUNK %d " % N.NEGQ_CHUNK in src and "#define CC_NEGQ_THREADS %d " % N.NEGQ_THREADS in src
