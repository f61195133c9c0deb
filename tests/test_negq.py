"""The exact order statistics of the negative compensated values, selected on the device (cc_negq_begin / _add_list / _select /
_end: k_negq_stage, the radix select of cc_negq.h), and what stands on them: Handle.negative_quantiles, fcs.estimate_logicle
with a handle, app.run on sidecars that hold "W": "estimate".  Every comparison is bit for bit against the referee of negq_util,
which restates the contract from numpy.  Shapes are the kernels' edges: n around a 64-event tile, d around a 64-dimension block,
slab seams at 64 and 128 events, every element type and byte order that has a kernel instance, the selection's own partition
(negq_util.NEGQ_CHUNK elements per workgroup of NEGQ_THREADS threads), and keys designed so that every digit pass decides."""
import ctypes
import json
import os

import numpy as np
import pytest

import fcs_util as F
import negq_util as N
import scenarios
import transform_util as U
from pipeline_util import knobs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

LITTLE, BIG = U.LITTLE, U.BIG
NS = (1, 63, 64, 65, 130, 200)
DS = (1, 5, 64, 65)
MS = (0, 3)
SLABS = (None, 64, 128)
TYPES = [(t, o) for t in (np.float32, np.float64, np.uint16, np.uint8, np.uint32) for o in (LITTLE, BIG)]  # (every kernel instance)
TIME_FIELDS = ("scan_ms", "run_ms", "comm_ms", "scan_ms_pruned", "calib_allgather_us", "calib_scan_ns_per_row_dim")
BAD_ARG = -2


@pytest.fixture(scope="module", params=SLABS, ids=lambda s: "slab%s" % s)
def handle(request):
    from chronoclust_amd import _lib
    env = {} if request.param is None else dict(CHRONOCLUST_HIP_INGEST_SLAB=request.param)
    with knobs(**env):
        h = _lib.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def plain():
    from chronoclust_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


def wants(d):
    """all, one dimension, every other dimension"""
    one = np.zeros(d, bool)
    one[d // 2] = True
    return (None, one, np.arange(d) % 2 == 0)


# ---- 1. against the referee -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
def test_count_lo_hi_frac_bit_for_bit(handle, n):
    compared = 0
    for di, d in enumerate(DS):
        for mi, m in enumerate(MS):
            dtype, order = TYPES[(NS.index(n) + 3 * di + 5 * mi) % len(TYPES)]
            lm = N.case(n, d, m, dtype, order, 100 * n + 10 * d + m)
            what = "%s %s %d x %d, m = %d" % (np.dtype(dtype).name, "big" if order == BIG else "little", n, d, m)
            before = handle.stats()
            for q in N.QS:
                exp = N.referee([lm], q)
                compared += int((exp[0] > 0).sum())
                N.same(handle.negative_quantiles([lm], q), exp, "%s, q = %g" % (what, q))
            for want in wants(d)[1:]:
                N.same(handle.negative_quantiles([lm], 0.05, want), N.referee([lm], 0.05, want), what + ", some wanted")
            assert handle.stats() == before, what
    assert compared >= 20, "hardly a negative value: nothing was compared"


def test_every_type_and_order_at_130_by_5(plain):
    for dtype, order in TYPES:
        for m in MS:
            lm = N.case(130, 5, m, dtype, order, 7 + m)
            exp = N.referee([lm], 0.05)
            assert m == 0 and np.dtype(dtype).kind == "u" or (exp[0] > 0).any()
            N.same(plain.negative_quantiles([lm], 0.05), exp, "%s %s, m = %d" % (np.dtype(dtype).name, order[0], m))


@pytest.mark.parametrize("q", N.QS)
def test_pooled_sources_with_spillovers_of_their_own(handle, q):
    from chronoclust_amd import _lib
    empty = _lib.ListMode(np.zeros(0, np.uint8), 0, 9, ">f4", columns=np.arange(5))
    a, b, c = N.case(130, 5, 3, np.float32, BIG, 1), N.case(65, 5, 3, np.uint16, LITTLE, 2), N.case(200, 5, 0, np.float64, BIG, 3)
    for pool in ([a], [a, b], [a, empty, b], [c, b, a], [empty]):
        for want in wants(5):
            N.same(handle.negative_quantiles(pool, q, want), N.referee(pool, q, want), "%d sources, q = %g" % (len(pool), q))


# ---- 2. designed keys -------------------------------------------------------------------------------------------------------------------

def test_designed_keys(handle):
    rec, names = N.designed_records()
    lm = U.list_mode(rec, LITTLE)
    got = {}
    for q in N.QS + (0.26,):
        got[q] = handle.negative_quantiles([lm], q)
        N.same(got[q], N.referee([lm], q), "designed keys, q = %g" % q)
    at = names.index
    count = got[0.05][0]
    assert [count[at("cnt %d" % k)] for k in range(3)] == [0, 1, 2]
    assert count[at("zeros")] == 2 and count[at("NaN")] == 39 and count[at("-Inf")] == 30
    for q in N.QS:  # no negative value: all zero, whatever q
        assert [float(got[q][k][at("cnt 0")]) for k in (1, 2, 3)] == [0.0, 0.0, 0.0]
    assert got[0.0][1][at("-Inf")] == -np.inf and got[0.0][2][at("-Inf")] == -29.0 and got[1.0][1][at("-Inf")] == -1.0
    tie = at("heavy ties")
    assert (got[0.05][1][tie], got[0.05][2][tie]) == (-5.0, -5.0)   # j and j + 1 inside one tie
    assert (got[0.25][1][tie], got[0.25][2][tie]) == (-5.0, -4.0)   # j on the last element of a tie
    assert (got[0.26][1][tie], got[0.26][2][tie]) == (-4.0, -4.0)   # j on the first of the next
    assert got[1.0][1][at("negative subnormals")] == -5e-324 and got[0.0][1][at("negative subnormals")] == -119 * 5e-324
    assert got[1.0][1][at("lowest mantissa byte")] == -1.0 and got[1.0][2][at("lowest mantissa byte")] == -1.0


# ---- 3. the seams of the selection's own partition -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", N.SEAM_NS)
def test_partition_seams(plain, n):
    rec = np.random.default_rng(n).normal(0.0, 100.0, (n, 2)).astype(np.float32)
    rec[n - 1] = (-1e9, -1e-9)  # the last element is the smallest of one column and the largest negative of the other
    lm = U.list_mode(rec, LITTLE)
    for q in (0.0, 0.05, 0.5, 1.0):
        N.same(plain.negative_quantiles([lm], q), N.referee([lm], q), "n = %d, q = %g" % (n, q))
    lo = plain.negative_quantiles([lm], 0.0)[1][0], plain.negative_quantiles([lm], 1.0)[1][1]
    assert lo == (np.float64(np.float32(-1e9)), np.float64(np.float32(-1e-9)))


# ---- 4. nothing observable moves --------------------------------------------------------------------------------------------------------

def lived(with_selection):
    """An upload, its run, a prefetch, the adopting upload, its run - with the selection run between each upload (or prefetch)
    and what follows it, or not - and everything a caller can observe afterwards."""
    import test_fcs_points as P
    from chronoclust_amd.clustering.hddstream import HDDStream
    cfg, Xs = P.stream(13, 300)
    lms = [U.list_mode(X, BIG) for X in Xs]
    other = [N.case(200, 5, 3, np.float32, BIG, 1), N.case(65, 5, 3, np.uint16, LITTLE, 2)]
    hdd = HDDStream(cfg, tuning=dict(sequential=1))
    h = hdd._h
    seen = []

    def select():
        if with_selection:
            N.same(h.negative_quantiles(other, 0.05), N.referee(other, 0.05), "between two calls")
            N.same(h.negative_quantiles([lms[0]], 0.5), N.referee([lms[0]], 0.5), "the resident source itself")

    hdd._set_dataset_dependent_parameters(lms[0])
    hdd._push_params()
    h.points_upload(lms[0])
    select()
    seen.append((h.points_download(13), h.points_download_xt(13)))
    h.online_run()
    seen.append(h.labels_download())
    h.points_prefetch(lms[1])
    select()
    h.points_upload(lms[1])
    select()
    seen.append((h.points_download(13), h.points_download_xt(13)))
    h.online_run()
    seen.append(h.labels_download())
    seen.append(tuple(h.export(kind)[key] for kind in (0, 1) for key in ("id", "uid", "w", "cf1", "cf2", "cen", "pref")))
    stats = {k: v for k, v in h.stats().items() if k not in TIME_FIELDS}
    out = [a.tobytes() for group in seen for a in group], h.counters(), stats
    h.close()
    return out


def test_nothing_observable_moves():
    a, b = lived(False), lived(True)
    assert a[1] == b[1], "counters"
    assert a[2] == b[2], "stats: %r" % {k: (a[2][k], b[2][k]) for k in a[2] if a[2][k] != b[2][k]}
    assert len(a[0]) == len(b[0]) == 22 and all(x == y for x, y in zip(a[0], b[0])), [i for i, (x, y) in enumerate(zip(a[0], b[0])) if x != y]
    assert a[2]["list_points"] == 600 and a[2]["windows"] > 0


# ---- 5. the C-ABI: select twice, every refusal ----------------------------------------------------------------------------------------

def c_select(h, q, d):
    from chronoclust_amd import _lib
    count, lo, hi, frac = np.empty(d, np.int64), np.empty(d), np.empty(d), np.empty(d)
    rc = h._lib.cc_negq_select(h._h, q, _lib._ptr(count, _lib._i64p), _lib._ptr(lo), _lib._ptr(hi), _lib._ptr(frac))
    return rc, (count, lo, hi, frac)


def test_select_twice_agrees_with_two_fresh_runs(plain):
    lm = N.case(200, 5, 3, np.float32, BIG, 4)
    desc, xf = lm.descriptor(), lm.transform_descriptor()
    lib, hh = plain._lib, plain._h
    assert lib.cc_negq_begin(hh, 5, None, 200) == 0
    assert lib.cc_negq_add_list(hh, ctypes.byref(desc), ctypes.byref(xf)) == 0
    for q in (0.05, 0.5, 0.05, 1.0, 0.0):
        rc, got = c_select(plain, q, 5)
        assert rc == 0
        N.same(got, N.referee([lm], q), "select again, q = %g" % q)
        fresh = plain_fresh(lm, q)
        assert np.array_equal(got[0], fresh[0]) and all(U.bits(a).tolist() == U.bits(b).tolist() for a, b in zip(got[1:], fresh[1:])), q
    assert lib.cc_negq_end(hh) == 0


def plain_fresh(lm, q):
    from chronoclust_amd import _lib
    h = _lib.Handle(0)
    try:
        return h.negative_quantiles([lm], q)
    finally:
        h.close()


def test_every_refusal_and_the_handle_works_afterwards(plain):
    from chronoclust_amd import _lib
    lib, hh = plain._lib, plain._h
    n, d = 130, 5
    lm = N.case(n, d, 3, np.float32, BIG, 9)
    desc, xf = lm.descriptor(), lm.transform_descriptor()
    p_desc, p_xf = ctypes.byref(desc), ctypes.byref(xf)
    plain.points_upload(lm)
    held = plain.points_download(d), plain.points_download_xt(d)
    before, counters = plain.stats(), plain.counters()
    out = np.empty(d, np.int64), np.empty(d), np.empty(d), np.empty(d)
    p_out = (_lib._ptr(out[0], _lib._i64p), _lib._ptr(out[1]), _lib._ptr(out[2]), _lib._ptr(out[3]))

    def refused(rc, reason):
        assert rc == BAD_ARG and reason in lib.cc_last_error(hh).decode(), (rc, reason, lib.cc_last_error(hh))

    # a null handle, null outputs
    assert lib.cc_negq_begin(None, d, None, n) == BAD_ARG and lib.cc_negq_add_list(None, p_desc, p_xf) == BAD_ARG
    assert lib.cc_negq_select(None, 0.05, *p_out) == BAD_ARG and lib.cc_negq_end(None) == BAD_ARG
    # without begin
    refused(lib.cc_negq_add_list(hh, p_desc, p_xf), "cc_negq_add_list without cc_negq_begin")
    refused(lib.cc_negq_select(hh, 0.05, *p_out), "cc_negq_select without cc_negq_begin")
    refused(lib.cc_negq_end(hh), "cc_negq_end without cc_negq_begin")
    # begin's own
    refused(lib.cc_negq_begin(hh, 0, None, n), "d must be in 1..1024")
    refused(lib.cc_negq_begin(hh, _lib.MAX_DIM + 1, None, n), "d must be in 1..1024")
    refused(lib.cc_negq_begin(hh, d, None, -1), "capacity must be non-negative")
    refused(lib.cc_negq_end(hh), "without cc_negq_begin")  # (a refused begin opened nothing)
    assert lib.cc_negq_begin(hh, d, None, n + 10) == 0
    for k in range(4):
        args = list(p_out)
        args[k] = None
        refused(lib.cc_negq_select(hh, 0.05, *args), "an output is null")
    for q in (-0.01, 1.01, float("nan"), float("inf")):
        refused(lib.cc_negq_select(hh, q, *p_out), "q must be in [0, 1]")
    # the source: another width, the capacity, and what cc_col_minmax_list_xf refuses about lm and xf
    narrow = N.case(20, d - 1, 0, np.float32, BIG, 1)
    refused(lib.cc_negq_add_list(hh, ctypes.byref(narrow.descriptor()), None), "cc_negq_begin was given 5")
    refused(lib.cc_negq_add_list(hh, None, p_xf), "the descriptor is null")

    def changed(struct, **fields):
        copy = type(struct).from_buffer_copy(struct)
        for k, v in fields.items():
            setattr(copy, k, v)
        return ctypes.byref(copy)

    refused(lib.cc_negq_add_list(hh, changed(desc, n=-1), p_xf), "n must be non-negative")
    refused(lib.cc_negq_add_list(hh, changed(desc, data=None), p_xf), "data is null")
    refused(lib.cc_negq_add_list(hh, changed(desc, dtype=_lib.DT_F16), p_xf), "dtype")
    refused(lib.cc_negq_add_list(hh, changed(desc, flags=2), p_xf), "unknown flag bits")
    refused(lib.cc_negq_add_list(hh, changed(desc, src_cols=0), p_xf), "src_cols must be in")
    refused(lib.cc_negq_add_list(hh, p_desc, changed(xf, reserved=1)), "reserved must be 0")
    refused(lib.cc_negq_add_list(hh, p_desc, changed(xf, m=_lib.MAX_COMP + 1)), "m must be in")
    refused(lib.cc_negq_add_list(hh, p_desc, changed(xf, comp=None)), "comp_cols or comp is null")
    twice = np.array([lm.transform.comp_cols[0]] * 3, np.int32)
    refused(lib.cc_negq_add_list(hh, p_desc, changed(xf, comp_cols=twice.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))), "repeats")
    nan = lm.transform.comp.copy()
    nan[1, 1] = np.nan
    refused(lib.cc_negq_add_list(hh, p_desc, changed(xf, comp=_lib._ptr(nan))), "is not finite")
    neg = np.full(d, -1.0)
    refused(lib.cc_negq_add_list(hh, p_desc, changed(xf, cofactor=_lib._ptr(neg))), "cofactor 0 is negative")
    assert lib.cc_negq_add_list(hh, changed(desc, n=0), p_xf) == 0  # (no event: accepted, adds nothing)
    assert lib.cc_negq_add_list(hh, p_desc, p_xf) == 0
    refused(lib.cc_negq_add_list(hh, p_desc, p_xf), "130 + 130 events exceed the capacity of 140")
    # the open selection took none of it: it holds the one source
    assert lib.cc_negq_select(hh, 0.05, *p_out) == 0
    N.same(out, N.referee([lm], 0.05), "behind the refusals")
    # begin while one is open starts over
    assert lib.cc_negq_begin(hh, d, None, n) == 0 and lib.cc_negq_select(hh, 0.05, *p_out) == 0
    assert out[0].tolist() == [0] * d and not any(U.bits(a).any() for a in out[1:])
    assert lib.cc_negq_end(hh) == 0
    refused(lib.cc_negq_end(hh), "without cc_negq_begin")
    # nothing moved
    assert plain.stats() == before and plain.counters() == counters
    U.same_bits(plain.points_download(d), held[0], "resident points")
    U.same_bits(plain.points_download_xt(d), held[1], "resident points, dimension-major")
    N.same(plain.negative_quantiles([lm], 0.25), N.referee([lm], 0.25), "afterwards")
    # cc_reset leaves an open selection alone
    assert lib.cc_negq_begin(hh, d, None, n) == 0 and lib.cc_negq_add_list(hh, p_desc, p_xf) == 0
    plain.reset()
    assert lib.cc_negq_select(hh, 0.5, *p_out) == 0
    N.same(out, N.referee([lm], 0.5), "across cc_reset")
    assert lib.cc_negq_end(hh) == 0


# ---- 6. estimate_logicle with a handle ------------------------------------------------------------------------------------------------

def test_estimate_logicle_with_a_handle_equals_without(tmp_path, handle, monkeypatch):
    import test_negq_cpu as C
    from chronoclust_amd import _lib, fcs
    paths = [C.write(tmp_path, "f%d.fcs" % i, kind, n, seed, spill_seed=seed)
             for i, (kind, n, seed) in enumerate([("f32", 200, 1), ("u16", 130, 2), ("f32", 0, 3), ("mixed", 90, 4)])]
    spec = {"CD3": {"W": "estimate"}, "CD4": {"W": "estimate", "q": 0.25, "M": 4}, "CD8": {"W": 0.5}}
    host = fcs.estimate_logicle(paths, columns=C.MARKERS, compensate=True, logicle=spec)
    src = C.sources_of(paths)
    a, b = N.referee(src, 0.05), N.referee(src, 0.25)
    assert host["CD3"]["W"] == N.width(a[0][0], a[4][0], 65536.0, 4.5) and host["CD4"]["W"] == N.width(b[0][1], b[4][1], 65536.0, 4.0)
    assert 0 < host["CD3"]["W"] < 2.25 and 0 < host["CD4"]["W"] < 2.0
    before = handle.stats()
    monkeypatch.setattr(_lib, "negative_quantiles_host", lambda *a, **kw: pytest.fail("the host route was taken"))
    assert fcs.estimate_logicle(paths, columns=C.MARKERS, compensate=True, logicle=spec, handle=handle) == host
    assert handle.stats() == before


# ---- 7. app.run end to end --------------------------------------------------------------------------------------------------------------

def test_app_run_resolves_the_sidecars_estimate(tmp_path, monkeypatch):
    from chronoclust_amd import _lib, app, fcs
    from test_app_end_to_end import _reset_logging
    n, d = 400, 5
    markers = ["CD%d" % i for i in range(d)]
    names = ["Time", markers[3], "FSC-A", markers[0], markers[4], "SSC-A", markers[1], markers[2]]
    comp_names = [markers[1], "FSC-A", markers[3]]  # (one compensated channel is not clustered on)
    spill = U.spillover(3, 8)[0]
    params = scenarios.blob_params(n)
    files = []
    for t in range(3):
        X = scenarios.make_blobs(900 + t, n, d, 8, 0.01)
        truth = np.zeros((n, len(names)), np.float32)
        for k, name in enumerate(markers):
            truth[:, names.index(name)] = (X[:, k] - 0.5) * 2000.0  # (half of the range below zero)
        truth[:, names.index("FSC-A")] = np.random.default_rng(t).uniform(0, 0.01, n)
        idx = [names.index(c) for c in comp_names]
        rec = truth.copy()
        rec[:, idx] = truth[:, idx] @ spill.astype(np.float32)
        rec.view(np.uint32)[:, names.index("Time")] = 0x7FC00000  # (a NaN pattern in a channel nobody reads)
        fn = os.path.join(str(tmp_path), "tp%d.fcs" % t)
        F.write_fcs(fn, F.fast_records(rec, BIG), len(names), "F", BIG, 32, names=names, tot=n, pad_before_data=t % 2, ranges=10000,
                    extra={"$SPILLOVER": U.spillover_text(comp_names, spill)})
        with open(fn + ".columns", "w") as f:
            f.write("\n".join(markers) + "\n")
        files.append(fn)
    # the referee's numbers: from the compensated events of all three files, pooled
    exp = N.referee([fcs.read_fcs(fn, columns=markers, compensate=True)[0] for fn in files], 0.05)
    assert (exp[0] >= 30).all()
    rows = {name: {"T": 10000.0, "W": N.width(exp[0][k], exp[4][k], 10000.0, 4.0), "M": 4.0, "A": 0.0} for k, name in enumerate(markers)}
    assert all(0.2 < row["W"] < 2.0 for row in rows.values()), rows

    def sidecars(logicle):
        for fn in files:
            with open(fn + ".transform", "w") as f:
                json.dump({"compensate": True, "logicle": logicle}, f)

    outs = []
    try:
        for what, logicle in (("resolved", rows), ("estimate", {"W": "estimate", "M": 4})):
            sidecars(logicle)
            out = os.path.join(str(tmp_path), "out_" + what)
            os.makedirs(out)
            if what == "estimate":  # the events are never decoded on the host, neither for the estimate nor for the run
                monkeypatch.setattr(_lib.ListMode, "__array__", lambda *a, **kw: pytest.fail("the events were decoded on the host"))
            app.run(data=files, output_directory=out, normalise_data=True, **params)
            outs.append(out)
            _reset_logging()
    finally:
        _reset_logging()
    for fn in ["result.csv"] + ["cluster_points_D%d.csv" % t for t in range(3)]:
        a, b = (open(os.path.join(o, fn), "rb").read() for o in outs)
        assert a == b and len(a) > 0, fn
    assert len(open(os.path.join(outs[1], "result.csv")).read().splitlines()) > 3, "no cluster was written: nothing was compared"
    assert not os.path.exists(os.path.join(outs[0], "logicle.json")), "a run that asks for no estimate writes no logicle.json"
    with open(os.path.join(outs[1], "logicle.json")) as f:
        assert json.load(f) == rows
    log = open(os.path.join(outs[1], "logs", "Chronoclust.log")).read()
    assert all("Logicle scale of channel %s estimated" % name in log for name in markers)
