"""List-mode event records compensated and arcsinh-transformed on the device (cc_points_upload_list_xf and its kin,
k_ingest_list_xf / k_col_minmax_list_xf).  The compensation is checked bit for bit against transform_util's restatement - an
explicit loop over j, elementwise numpy only - on inputs that first prove, on the CPU, that they tell the specified order
from a fused and from a descending sum; the two resident copies, the column reduction and the scaled upload hold one value
everywhere; asinh is held to its measured distance from an extended-precision reference; the online phase, the read-only
assignment and a group of two cannot tell the transformed records from their own read-back handed over as float64; a prefetch
is adopted by content of the transform; every malformed transform is refused before anything runs; app.run on `.fcs`
timepoints with `.transform` sidecars writes the files of the run over the read-back.
Shapes are the kernel's edges: n around a 64-event tile, d around a 64-dimension block, m from none to CC_MAX_COMP, slab
seams at 64 and 128 events."""
import ctypes
import json
import os

import numpy as np
import pytest

import assign_util as A
import fcs_util as F
import scenarios
import table_util as T
import transform_util as U
from pipeline_util import knobs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

LITTLE, BIG = U.LITTLE, U.BIG
NS = (1, 63, 64, 65, 130, 200)
DS = (1, 5, 64, 65)
MS = (0, 1, 2, 9, 64)
SLABS = (None, 64, 128)
TYPES = [(t, o) for t in (np.float32, np.float64, np.uint16, np.uint8, np.uint32) for o in (LITTLE, BIG)]  # (every kernel instance)
# The largest distance, in units in the last place, of the device's asinh from the extended-precision reference over
# |q| in [1e-9, 1e6], both signs and 0, measured on the MI355X (profiles/ingest_transform.txt); the bound of every comparison
# against that reference is this plus 1 ulp for the reference's own rounding.
ASINH_MEASURED_MAX_ULP = 1
ASINH_BOUND_ULP = ASINH_MEASURED_MAX_ULP + 1


def layout(d, m, seed, repeat=True, all_selected=False):
    """(src_cols, cols, comp_cols) with every arrangement at once where d and m leave room: about half of the selected
    dimensions are compensated columns - so compensated columns stay unselected and selected ones uncompensated -, in an order
    that is not the matrix's, and the last selected dimension repeats the first."""
    rng = np.random.default_rng(seed)
    src_cols = d + m + 2
    perm = rng.permutation(src_cols)
    comp_cols = perm[:m]
    k = min(m, d if all_selected else (d + 1) // 2)
    cols = np.concatenate([rng.permutation(comp_cols)[:k], perm[m:m + d - k]]).astype(np.int64)
    rng.shuffle(cols)
    if repeat and d > 1:
        cols[-1] = cols[0]
    return src_cols, cols, comp_cols.astype(np.int64)


def case(n, d, m, dtype, order, seed, cofactor=None, zeros=False, **kw):
    """A ListMode with its transform and the restatement's compensated values (cofactors not applied).  zeros: +0.0 and
    -0.0 in the first and last event of a selected floating channel that is not compensated and has a cofactor."""
    from chronoclust_amd import _lib
    src_cols, cols, comp_cols = layout(d, m, seed, **kw)
    rec = U.records(dtype, n, src_cols, seed + 1)
    if zeros and np.dtype(dtype).kind == "f":
        free = [k for k, col in enumerate(cols) if col not in comp_cols and cofactor[k] > 0]
        if free:
            rec[0, cols[free[0]]], rec[n - 1, cols[free[0]]] = 0.0, -0.0
    masks = None
    if np.dtype(dtype).kind == "u":
        masks = [(0x7FFF, 0x3FF, 0xFFFFFFFF, 0xFFF)[c % 4] for c in range(d)]
        if d > 1:
            masks[-1] = masks[0]  # (the repeated column under one mask: its compensated input is decoded once)
    inv = U.spillover(m, seed + 2)[1] if m else None
    if m == 0 and cofactor is None:
        cofactor = np.zeros(d)  # (cofactors of 0 pass through: the transform's kernel without a transform to apply)
    tr = _lib.ListTransform(comp_cols if m else None, inv, cofactor)
    lm = U.list_mode(rec, order, cols, masks, tr)
    x = U.decoded(rec, cols, masks)
    xs = U.comp_inputs(rec, cols, masks, comp_cols)
    exp = U.compensated(x, xs, cols, comp_cols, inv) if m else x
    return dict(lm=lm, rec=rec, cols=cols, comp_cols=comp_cols, masks=masks, inv=inv, x=x, xs=xs, exp=exp, transform=tr)


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


def resident(h, d):
    return h.points_download(d), h.points_download_xt(d)


def one_value(h, d, what):
    """Both resident copies hold the same doubles, the pad rows +0.0; returns the row-major copy."""
    from chronoclust_amd import _lib
    x, xt = resident(h, d)
    assert xt.shape == (_lib.xt_rows(d), x.shape[0]), what
    U.same_bits(xt[:d], x.T, what + ": dimension-major against row-major")
    assert not U.bits(xt[d:]).any(), what + ": pad rows"
    return x


# ---- 1. compensation is bit for bit ---------------------------------------------------------------------------------------------

def test_the_inputs_tell_the_orders_apart():
    """CPU part of (1): on the 130 x 9 case at least 10 % of the expected elements differ from the sum with every step fused
    (exact, fractions.Fraction) and from the sum in descending j - else a kernel that contracts or reorders would pass."""
    for dtype, order in TYPES:
        c = case(130, 9, 9, dtype, order, 11, all_selected=True, repeat=False)
        fused = U.compensated_fused(c["x"], c["xs"], c["cols"], c["comp_cols"], c["inv"])
        desc = U.compensated(c["x"], c["xs"], c["cols"], c["comp_cols"], c["inv"], descending=True)
        for what, other in (("fused", fused), ("descending", desc)):
            share = float((U.bits(other) != U.bits(c["exp"])).mean())
            print("%s %s: %.0f %% of the expected elements differ from the %s sum" % (np.dtype(dtype).name, order[0], 100 * share, what))
            assert share >= 0.10, (np.dtype(dtype).name, what, share)


@pytest.mark.parametrize("n", NS)
def test_compensation_is_bit_for_bit(handle, n):
    seen = set()
    for di, d in enumerate(DS):
        for mi, m in enumerate(MS):
            ti = (NS.index(n) + di + 2 * mi) % len(TYPES)
            dtype, order = TYPES[ti]
            c = case(n, d, m, dtype, order, 100 * n + 10 * d + m)
            what = "%s %s %d x %d, m = %d" % (np.dtype(dtype).name, "big" if order == BIG else "little", n, d, m)
            if m >= 3 and n >= 63:
                # (of the compensated dimensions' elements, a tenth at least is another double when summed from the other end)
                desc = U.compensated(c["x"], c["xs"], c["cols"], c["comp_cols"], c["inv"], descending=True)
                hit = np.isin(c["cols"], c["comp_cols"])
                assert (U.bits(desc)[:, hit] != U.bits(c["exp"])[:, hit]).mean() >= 0.10, what
            before = handle.stats()["list_points"]
            handle.points_upload(c["lm"])
            assert handle.stats()["list_points"] == before + n, what
            U.same_bits(one_value(handle, d, what), c["exp"], what)
            U.same_bits(np.asarray(c["lm"]), c["exp"], what + ": ListMode's host transform")
            seen.add(ti)
    assert len(seen) == len(TYPES)


def test_the_130_by_9_case_of_every_type(plain):
    """The very inputs test_the_inputs_tell_the_orders_apart vouches for."""
    for dtype, order in TYPES:
        c = case(130, 9, 9, dtype, order, 11, all_selected=True, repeat=False)
        plain.points_upload(c["lm"])
        U.same_bits(one_value(plain, 9, np.dtype(dtype).name), c["exp"], "%s %s 130 x 9" % (np.dtype(dtype).name, order[0]))


# ---- 2. one value, everywhere -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", NS)
def test_one_value_everywhere(handle, n):
    from chronoclust_amd.scaling.scaler import Scaler
    for di, d in enumerate(DS):
        for mi, m in enumerate(MS):
            dtype, order = TYPES[(NS.index(n) + di + mi) % len(TYPES)]
            cof = np.where(np.arange(d) % 3 == 1, 0.0, (5.0, 150.0)[mi % 2])  # (cofactor 0 on every third channel)
            c = case(n, d, m, dtype, order, 7000 + 100 * n + 10 * d + m, cofactor=cof, zeros=True)
            what = "%s %s %d x %d, m = %d" % (np.dtype(dtype).name, "big" if order == BIG else "little", n, d, m)
            lm = c["lm"]
            handle.points_upload(lm)
            x = one_value(handle, d, what)
            assert np.isfinite(x).all(), what
            ref = U.with_cofactors(c["exp"], cof)
            dist = U.ulp_distance(x, ref)
            assert dist.max() <= ASINH_BOUND_ULP, "%s: %d ulp from the reference" % (what, dist.max())
            passed = cof == 0.0
            U.same_bits(x[:, passed], c["exp"][:, passed], what + ": cofactor 0 passes through")
            zero = (c["exp"] == 0.0) & ~passed[None, :]
            assert (x[zero] == 0.0).all(), what + ": asinh(+-0)"
            # the column reduction: the very doubles the upload holds (== : the sign of a zero is free)
            before = handle.stats()["list_points"]
            mn, mx = handle.col_minmax(lm)
            assert handle.stats()["list_points"] == before, what
            assert np.array_equal(mn, x.min(axis=0)) and np.array_equal(mx, x.max(axis=0)), what + ": col_minmax"
            # the scaler's fit on it: the scaled upload is numpy's two roundings, the column minimum lands on 0.0
            sc = Scaler()
            sc._finish_fit(mn.copy(), mx.copy())
            handle.points_upload_scaled(lm, sc.scale_, sc.min_)
            xs = one_value(handle, d, what + ", scaled")
            U.same_bits(xs, x * sc.scale_ + sc.min_, what + ": scaled upload")
            assert (xs.min(axis=0) == 0.0).all(), what + ": the column minimum under the scaler's fit"
            assert np.isfinite(xs).all(), what


# ---- 3. asinh against numpy -----------------------------------------------------------------------------------------------------------

def sweep():
    """q over |q| in [1e-9, 1e6], log-uniform per three decades, both signs, and 0: [n, 4] float64, with the cofactor."""
    rng = np.random.default_rng(3)
    q = np.concatenate([10.0 ** rng.uniform(lo, lo + 3, 20000) for lo in (-9, -6, -3, 0, 3)])
    q = np.concatenate([q, -q, [0.0, -0.0, 1e-9, -1e-9, 1e6, -1e6, 1.0, -1.0]])
    c = 5.0
    v = q * c
    return np.ascontiguousarray(v.reshape(-1, 4)), c


def test_asinh_against_the_extended_precision_reference(plain):
    from chronoclust_amd import _lib
    v, c = sweep()
    lm = U.list_mode(v, LITTLE, None, None, _lib.ListTransform(cofactor=c))
    plain.points_upload(lm)
    got = one_value(plain, 4, "sweep")
    q = np.divide(v, c)
    assert np.abs(q[q != 0]).min() <= 1.1e-9 and np.abs(q).max() >= 0.9e6
    ref = U.asinh_reference(q)
    dist = U.ulp_distance(got, ref)
    for lo in (-9, -6, -3, 0, 3):
        band = (np.abs(q) >= 10.0 ** lo) & (np.abs(q) < 10.0 ** (lo + 3))
        print("|q| in [1e%d, 1e%d): largest distance %d ulp, %.2f %% of %d values off by one or more"
              % (lo, lo + 3, dist[band].max(), 100.0 * (dist[band] > 0).mean(), band.sum()))
    print("asinh on the device: largest distance from the reference %d ulp over %d values" % (dist.max(), dist.size))
    assert (got[q == 0] == 0).all()
    assert dist.max() <= ASINH_BOUND_ULP
    # compensated values through the same division and asinh: v bit for bit from the restatement
    cs = case(130, 9, 9, np.float32, BIG, 11, cofactor=np.full(9, 150.0), all_selected=True, repeat=False)
    plain.points_upload(cs["lm"])
    dist = U.ulp_distance(one_value(plain, 9, "compensated"), U.with_cofactors(cs["exp"], np.full(9, 150.0)))
    print("compensated 130 x 9, cofactor 150: largest distance %d ulp" % dist.max())
    assert dist.max() <= ASINH_BOUND_ULP


# ---- 4. downstream does not notice --------------------------------------------------------------------------------------------------

def raw_for(X, seed, cofactor=5.0, extra=4):
    """Big-endian float64 records whose transform gives (about) X: sinh(X) * cofactor, the first half of the dimensions spilled
    into each other, `extra` channels of NaN between them.  Returns the ListMode."""
    from chronoclust_amd import _lib
    n, d = X.shape
    rng = np.random.default_rng(seed)
    m = max(1, min(d // 2, 9))
    spill, inv = U.spillover(m, seed)
    perm = rng.permutation(d + extra)
    cols = perm[:d]
    truth = np.sinh(X) * cofactor
    truth[:, :m] = truth[:, :m] @ spill  # (building an input: any rounding will do)
    rec = np.full((n, d + extra), np.nan)
    rec[:, cols] = truth
    return U.list_mode(rec, BIG, cols, None, _lib.ListTransform(cols[:m], inv, cofactor))


def read_back(lm):
    from chronoclust_amd import _lib
    h = _lib.Handle(0)
    try:
        h.points_upload(lm)
        return h.points_download(lm.shape[1])
    finally:
        h.close()


@pytest.mark.parametrize("d,prune", [(5, None), (13, None), (13, 2)])
def test_the_online_phase_does_not_notice(d, prune):
    import test_fcs_points as P
    n = 300
    cfg, Xs = P.stream(d, n)
    lms = [raw_for(X, 50 + t) for t, X in enumerate(Xs)]
    backs = [read_back(lm) for lm in lms]
    assert all(np.abs(b - X).max() < 1e-9 for b, X in zip(backs, Xs)), "the records do not hold the blobs"
    with knobs(**({} if prune is None else dict(CHRONOCLUST_HIP_PRUNE=prune))):
        _, exp = P.run_stream(cfg, backs)
        _, got = P.run_stream(cfg, lms)
    P.same_run(got, exp, "d=%d prune=%s" % (d, prune), np.cumsum([n, n]).tolist())
    assert len(set(got[-1]["path"].tolist())) > 1, "every point took one path: nothing was compared"


def test_assign_with_a_chunk_of_100_does_not_notice():
    import test_fcs_points as P
    from chronoclust_amd import _lib
    cfg, Xs = P.stream(13, 300)
    with knobs(CHRONOCLUST_HIP_ASSIGN_CHUNK=100, CHRONOCLUST_HIP_INGEST_SLAB=64):
        hdd, _ = P.run_stream(cfg, [Xs[0]])
    h = hdd._h
    q = np.vstack([Xs[0][:100], Xs[1][:65]])
    lm = raw_for(q, 9)
    back = read_back(lm)
    exp = h.assign(back, want_dist=True)
    before = h.stats()
    got = h.assign(lm, want_dist=True)
    after = h.stats()
    A.same_assign(got, exp, "transformed records")
    U.same_bits(got[2], exp[2], "dist")
    assert after["assign_launches"] == 2 and after["assign_points"] == 165
    assert after["list_points"] == before["list_points"] + 165
    assert len(set(got[1].tolist())) > 1, "the queries all took one path: nothing was compared"


def test_a_group_of_two_does_not_notice():
    pcores, outliers, par, X, meta = T.build_online("stale-3000+1096x20")
    from chronoclust_amd import _lib
    lm = raw_for(X, 21)
    back = read_back(lm)
    assert np.abs(back - X).max() < 1e-9
    h = _lib.Handle(0)
    try:
        single = T.handle_online(h, (pcores, outliers, par, back, meta))
        lists = [h.export(kind) for kind in (0, 1)]
        counters = h.counters()
    finally:
        h.close()
    hs, labels, stats = T.group_online(2, (pcores, outliers, par, lm, meta))
    try:
        for rank in range(2):
            for key, a, b in (("uid", labels[rank][0][0], single[0][0]), ("path", labels[rank][0][1], single[0][1])):
                diff = T._first_diff(a, b)
                assert diff is None, "rank %d %s: %s" % (rank, key, diff)
            for kind in (0, 1):
                got = hs[rank].export(kind)
                for key in T.KEYS:
                    assert got[key].tobytes() == lists[kind][key].tobytes(), (rank, kind, key)
            assert hs[rank].counters() == counters
            assert stats[rank]["list_points"] == len(X) and stats[rank]["sharded_windows"] > 0, stats[rank]
    finally:
        for g in hs:
            g.close()


# ---- 5. prefetch ----------------------------------------------------------------------------------------------------------------------

def test_prefetch_is_adopted_by_the_same_transform_only(handle):
    from chronoclust_amd import _lib
    n, d, m = 200, 13, 9
    c = case(n, d, m, np.float32, BIG, 77, cofactor=np.full(d, 5.0))
    lm, rec, cols = c["lm"], c["rec"], c["cols"]

    def variant(transform):
        return _lib.ListMode(lm.buffer, n, lm.src_cols, lm.dtype, columns=cols, transform=transform)

    def values(v):
        handle.points_upload(v)
        return handle.points_download(d)

    own = values(lm)
    before = handle.stats()["list_points"]
    handle.points_prefetch(lm)
    handle.points_upload(lm)  # adopted
    assert handle.stats()["list_points"] == before + n
    U.same_bits(one_value(handle, d, "prefetched"), own, "prefetched")
    # an equal transform built anew: adopted too
    handle.points_prefetch(lm)
    handle.points_upload(variant(_lib.ListTransform(c["comp_cols"].copy(), c["inv"].copy(), np.full(d, 5.0))))
    U.same_bits(handle.points_download(d), own, "an equal transform")
    other_inv = c["inv"].copy()
    other_inv[4, 2] *= 1.5  # (one matrix entry)
    other_cof = np.full(d, 5.0)
    other_cof[d - 2] = 6.0
    swapped_cols = c["comp_cols"].copy()
    swapped_cols[[0, 1]] = swapped_cols[[1, 0]]
    variants = {"one matrix entry": variant(_lib.ListTransform(c["comp_cols"], other_inv, np.full(d, 5.0))),
                "one cofactor": variant(_lib.ListTransform(c["comp_cols"], c["inv"], other_cof)),
                "the compensated columns": variant(_lib.ListTransform(swapped_cols, c["inv"], np.full(d, 5.0))),
                "no cofactors": variant(_lib.ListTransform(c["comp_cols"], c["inv"])),
                "no transform": variant(None)}
    for what, other in variants.items():
        assert other._bytes.ctypes.data == lm._bytes.ctypes.data
        want = values(other)
        assert not np.array_equal(want, own), what
        for first, second, exp in ((lm, other, want), (other, lm, own)):
            handle.points_prefetch(first)
            handle.points_upload(second)  # discarded: another transform
            U.same_bits(one_value(handle, d, what), exp, "only %s differs" % what)
    # scaled prefetch with a transform, adopted; the same scaling without the transform is another upload
    scale, min_ = np.full(d, 0.25), np.full(d, 0.5)
    handle.points_prefetch(lm, scale, min_)
    handle.points_upload_scaled(lm, scale, min_)
    U.same_bits(handle.points_download(d), own * scale + min_, "scaled prefetch")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------

def test_transform_refusals(plain):
    from chronoclust_amd import _lib
    handle = plain
    n, d, m = 40, 6, 3
    c = case(n, d, m, np.float32, BIG, 5, cofactor=np.full(d, 5.0))
    lm = c["lm"]
    handle.points_upload(lm)
    held = resident(handle, d)
    desc = lm.descriptor()
    i32, f64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)

    def xf(**over):
        out = lm.transform_descriptor()
        for k, v in over.items():
            setattr(out, k, v)
        return out

    def ints(v):
        a = np.array(v, np.int32)
        keep.append(a)
        return a.ctypes.data_as(i32)

    def doubles(v):
        a = np.array(v, np.float64)
        keep.append(a)
        return a.ctypes.data_as(f64)

    keep = []
    cc = c["comp_cols"].tolist()
    inv = c["inv"].ravel().tolist()
    big = np.eye(65).ravel()
    cases = [("m < 0", xf(m=-1), "m must be"),
             ("m = 65", xf(m=65, comp_cols=ints(list(range(65))), comp=doubles(big)), "m must be"),
             ("null comp_cols", xf(comp_cols=None), "null"),
             ("null comp", xf(comp=None), "null"),
             ("a column beyond the record", xf(comp_cols=ints([cc[0], lm.src_cols, cc[2]])), "compensated column %d" % lm.src_cols),
             ("a negative column", xf(comp_cols=ints([cc[0], -1, cc[2]])), "compensated column -1"),
             ("a column that repeats", xf(comp_cols=ints([cc[0], cc[1], cc[0]])), "repeats"),
             ("a NaN matrix entry", xf(comp=doubles(inv[:4] + [np.nan] + inv[5:])), "not finite"),
             ("an infinite matrix entry", xf(comp=doubles(inv[:8] + [np.inf])), "not finite"),
             ("a negative cofactor", xf(cofactor=doubles([5, 5, -1, 5, 5, 5])), "cofactor 2"),
             ("a NaN cofactor", xf(cofactor=doubles([5, 5, 5, 5, 5, np.nan])), "cofactor 5"),
             ("an infinite cofactor", xf(cofactor=doubles([np.inf, 5, 5, 5, 5, 5])), "cofactor 0"),
             ("reserved", xf(reserved=1), "reserved")]
    before = handle.stats()
    mn, mx = np.zeros(d), np.zeros(d)
    uid, path = np.zeros(n, np.int64), np.zeros(n, np.int8)
    lib, hh = handle._lib, handle._h
    for what, t, reason in cases:
        calls = [lib.cc_points_upload_list_xf(hh, ctypes.byref(desc), ctypes.byref(t), None, None),
                 lib.cc_points_prefetch_list_xf(hh, ctypes.byref(desc), ctypes.byref(t), None, None),
                 lib.cc_col_minmax_list_xf(hh, ctypes.byref(desc), ctypes.byref(t), _lib._ptr(mn), _lib._ptr(mx)),
                 lib.cc_online_list_xf(hh, ctypes.byref(desc), ctypes.byref(t), _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p)),
                 lib.cc_assign_list_xf(hh, ctypes.byref(desc), ctypes.byref(t), _lib._ptr(uid, _lib._i64p), _lib._ptr(path, _lib._i8p), None)]
        assert calls == [-2] * 5, (what, calls)  # CC_ERR_BAD_ARG
        assert reason in lib.cc_last_error(hh).decode(), (what, lib.cc_last_error(hh))
    # the sibling's refusals stand beside them
    bad_desc = lm.descriptor()
    bad_desc.src_cols = 0
    good = xf()
    assert lib.cc_points_upload_list_xf(hh, ctypes.byref(bad_desc), ctypes.byref(good), None, None) == -2
    assert lib.cc_points_upload_list_xf(hh, ctypes.byref(desc), ctypes.byref(good), _lib._ptr(mn), None) == -2
    # through Python: a ValueError
    with pytest.raises(ValueError, match="bad argument"):
        handle.points_upload(_lib.ListMode(lm.buffer, n, lm.src_cols, lm.dtype, columns=c["cols"],
                                           transform=_lib.ListTransform(c["comp_cols"], c["inv"], -1.0)))
    # nothing moved, nothing was launched or counted
    after = handle.stats()
    for key in ("list_points", "view_points", "f32_points", "assign_launches", "assign_points", "scan_launches", "scan_u_launches",
                "scan_p_launches", "windows", "points"):
        assert after[key] == before[key], key
    x, xt = resident(handle, d)
    U.same_bits(x, held[0], "resident points behind refused calls")
    U.same_bits(xt, held[1], "resident points behind refused calls, dimension-major")
    # xf NULL, and a transform that asks for nothing, are the sibling
    plain_lm = _lib.ListMode(lm.buffer, n, lm.src_cols, lm.dtype, columns=c["cols"])
    nothing = _lib.CcListTransform(0, 0, None, None, None)
    for t in (None, ctypes.byref(nothing)):
        handle._check(lib.cc_points_upload_list_xf(hh, ctypes.byref(desc), t, None, None))
        U.same_bits(handle.points_download(d), np.asarray(plain_lm, np.float64), "no transform")


def test_nan_in_a_compensated_column_is_refused_and_elsewhere_is_not(plain):
    from chronoclust_amd import _lib
    n, d, m = 130, 5, 9
    for dtype in (np.float32, np.float64):
        c = case(n, d, m, dtype, BIG, 31, cofactor=np.full(d, 5.0))
        src_cols = c["rec"].shape[1]
        unselected_comp = [int(v) for v in c["comp_cols"] if v not in c["cols"]]
        neither = [v for v in range(src_cols) if v not in c["cols"] and v not in c["comp_cols"]]
        assert unselected_comp and neither
        plain.points_upload(c["lm"])
        clean = plain.points_download(d)
        for value in (np.nan, np.inf):
            rec = c["rec"].copy()
            rec[100, neither[0]] = value
            lm = U.list_mode(rec, BIG, c["cols"], None, c["transform"])
            plain.points_upload(lm)  # neither selected nor compensated: never read
            U.same_bits(plain.points_download(d), clean, "a %r in a channel that is neither selected nor compensated" % value)
            rec[100, unselected_comp[0]] = value
            lm = U.list_mode(rec, BIG, c["cols"], None, c["transform"])
            with pytest.raises(ValueError, match="non-finite"):
                plain.points_upload(lm)
            plain.points_prefetch(lm)
            with pytest.raises(ValueError, match="non-finite"):
                plain.points_upload(lm)


# ---- 8. app.run end to end --------------------------------------------------------------------------------------------------------------

def test_app_run_on_fcs_timepoints_with_transform_sidecars(tmp_path, monkeypatch):
    from chronoclust_amd import _lib, app, fcs
    from test_app_end_to_end import _reset_logging
    n, d = 400, 5
    markers = ["CD%d" % i for i in range(d)]
    names = ["Time", markers[3], "FSC-A", markers[0], markers[4], "SSC-A", markers[1], markers[2]]
    comp_names = [markers[1], "FSC-A", markers[3]]  # (one compensated channel is not clustered on)
    spill = U.spillover(3, 8)[0]
    params = scenarios.blob_params(n)
    files, backs = [], []
    for t in range(3):
        X = scenarios.make_blobs(900 + t, n, d, 8, 0.01)
        truth = np.zeros((n, len(names)), np.float32)
        for k, name in enumerate(markers):
            truth[:, names.index(name)] = np.sinh(X[:, k]) * 5.0
        truth[:, names.index("FSC-A")] = np.random.default_rng(t).uniform(0, 0.01, n)
        idx = [names.index(c) for c in comp_names]
        rec = truth.copy()
        rec[:, idx] = truth[:, idx] @ spill.astype(np.float32)
        rec.view(np.uint32)[:, names.index("Time")] = 0x7FC00000  # (a NaN pattern in a channel nobody reads)
        fn = os.path.join(str(tmp_path), "tp%d.fcs" % t)
        F.write_fcs(fn, F.fast_records(rec, BIG), len(names), "F", BIG, 32, names=names, tot=n, pad_before_data=t % 2,
                    extra={"$SPILLOVER": U.spillover_text(comp_names, spill)})
        with open(fn + ".columns", "w") as f:
            f.write("\n".join(markers) + "\n")
        with open(fn + ".transform", "w") as f:
            json.dump({"compensate": True, "cofactor": 5}, f)
        files.append(fn)
        lm = fcs.read_fcs(fn, columns=markers, compensate=True, cofactor=5)[0]
        assert isinstance(lm, _lib.ListMode) and lm.transform is not None and lm.transform.m == 3
        backs.append(read_back(lm))
        assert np.abs(backs[-1] - X).max() < 1e-4
    npys = []
    for t, b in enumerate(backs):
        fn = os.path.join(str(tmp_path), "tp%d.npy" % t)
        np.save(fn, b)
        with open(fn + ".columns", "w") as f:
            f.write("\n".join(markers) + "\n")
        npys.append(fn)
    seen, made = [], []

    class Recording(app.HDDStream):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

        def online_microcluster_maintenance(self, input_dataset, *a, **kw):
            seen.append(input_dataset)
            return super().online_microcluster_maintenance(input_dataset, *a, **kw)

    outs = []
    try:
        out = os.path.join(str(tmp_path), "out_npy")
        os.makedirs(out)
        app.run(data=npys, output_directory=out, normalise_data=True, **params)
        outs.append(out)
        _reset_logging()
        # the events of the .fcs run are never decoded on the host: ListMode's host decode is out of reach during it
        monkeypatch.setattr(app, "HDDStream", Recording)
        monkeypatch.setattr(_lib.ListMode, "__array__", lambda *a, **kw: pytest.fail("the events were decoded on the host"))
        out = os.path.join(str(tmp_path), "out_fcs")
        os.makedirs(out)
        app.run(data=files, output_directory=out, normalise_data=True, **params)
        outs.append(out)
    finally:
        _reset_logging()
    assert len(seen) == 3 and all(isinstance(x, _lib.ListMode) and x.transform is not None for x in seen)
    stats = made[0].stats()
    assert stats["list_points"] >= 3 * n and stats["view_points"] == 0 and stats["f32_points"] == 0
    for fn in ["result.csv"] + ["cluster_points_D%d.csv" % t for t in range(3)]:
        a, b = (open(os.path.join(o, fn), "rb").read() for o in outs)
        assert a == b and len(a) > 0, fn
    assert len(open(os.path.join(outs[1], "result.csv")).read().splitlines()) > 3, "no cluster was written: nothing was compared"
