"""One comparison decides for every kind of source whether an upload adopts a prefetch (IngestSrc::same, cc_ingest_src.h): the
kind first, then that kind's fields.  Four readings of ONE buffer at ONE address with the same n and d - float32 rows, a
columns-form view, little-endian event records with the channels reversed, big-endian event records - widen to four different
arrays; a prefetch of one followed by the upload of another must discard what was fetched and leave the second's values, and
only the second's counter moves.  Once on pieces of the default size (one piece) and once, in a child process, with
CHRONOCLUST_HIP_INGEST_SLAB=64 (the knob is read when a handle is created; the worker then runs two pieces)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

N, D = 128, 16
KINDS = ("float32 rows", "columns-form view", "little-endian records, channels reversed", "big-endian records")
COUNTER = {KINDS[0]: "f32_points", KINDS[1]: "view_points", KINDS[2]: "list_points", KINDS[3]: "list_points"}
PAIRS = list(itertools.product(range(4), repeat=2))  # (first, second): the 12 ordered pairs and the 4 "same reading" cases


def readings():
    """{kind: (what the library is given, its widened values)} over one buffer.  Bytes 1 .. 126: the exponent field of a float32
    is all ones in neither byte order, so every reading is finite."""
    from chronoclust_amd import _lib
    buf = np.random.default_rng(20261019).integers(1, 127, N * D * 4, dtype=np.uint8)
    rows = buf.view(np.float32).reshape(N, D)
    given = (rows, buf.view(np.float32).reshape(D, N).T,
             _lib.ListMode(buf, N, D, "<f4", columns=np.arange(D - 1, -1, -1)), _lib.ListMode(buf, N, D, ">f4"))
    assert _lib.is_f32_points(given[0]) and _lib.points_source(given[1])[1] is not None
    assert all(g.shape == (N, D) for g in given)
    assert given[1].ctypes.data == rows.ctypes.data and all(g._bytes.ctypes.data == rows.ctypes.data for g in given[2:])
    wide = [np.ascontiguousarray(np.asarray(g, dtype=np.float64)) for g in given]
    assert all(np.isfinite(w).all() for w in wide)
    assert not any(np.array_equal(a, b) for a, b in itertools.combinations(wide, 2))
    return dict(zip(KINDS, zip(given, wide)))


def check_pair(h, src, first, second):
    """points_prefetch(first) then points_upload(second): the resident copies are the widened `second`, bit for bit, and of
    the three counters only second's advances, by N."""
    from chronoclust_amd import _lib
    what = "prefetch of %s, upload of %s" % (first, second)
    before = h.stats()
    h.points_prefetch(src[first][0])
    h.points_upload(src[second][0])
    after = h.stats()
    for key in ("f32_points", "view_points", "list_points"):
        assert after[key] - before[key] == (N if key == COUNTER[second] else 0), (what, key)
    exp = src[second][1]
    x, xt = h.points_download(D), h.points_download_xt(D)
    assert np.array_equal(x.view(np.int64), exp.view(np.int64)), what + ": row-major copy"
    assert xt.shape == (_lib.xt_rows(D), N), what
    assert np.array_equal(xt[:D].view(np.int64), np.ascontiguousarray(exp.T).view(np.int64)), what + ": dimension-major copy"
    assert not xt[D:].view(np.int64).any(), what + ": pad rows"


def check_all_pairs():
    """Every pair on a handle of its own (the child process's entry)."""
    from chronoclust_amd import _lib
    src = readings()
    h = _lib.Handle(0)
    try:
        for a, b in PAIRS:
            check_pair(h, src, KINDS[a], KINDS[b])
    finally:
        h.close()


@pytest.fixture(scope="module")
def sources():
    return readings()


@pytest.fixture(scope="module")
def handle():
    from chronoclust_amd import _lib
    h = _lib.Handle(0)
    yield h
    h.close()


@pytest.mark.parametrize("first,second", PAIRS, ids=["%d-then-%d" % p for p in PAIRS])
def test_prefetch_of_one_reading_upload_of_another(handle, sources, first, second):
    check_pair(handle, sources, KINDS[first], KINDS[second])


def test_the_same_pairs_in_two_pieces():
    """CHRONOCLUST_HIP_INGEST_SLAB=64: a prefetch is two pieces, an upload two slabs."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_ingest_kinds as t; t.check_all_pairs(); print('all pairs ok')" \
           % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=100,
                       env=dict(os.environ, CHRONOCLUST_HIP_INGEST_SLAB="64"))
    assert r.returncode == 0 and "all pairs ok" in r.stdout, r.stdout + r.stderr
