"""CPU tests of the width rule of the snapshot scans (cc::scan_width of csrc/cc_batch.h through cc_scan_width): at which
padded width the scan kernels run for a stream of d dimensions, whether the plain scan is the scalar-operand kernel
(k_scan_u) and which pruned chain exists - before any CHRONOCLUST_HIP_* knob.  No GPU.  Every expected value is written
out by hand from the rule:
  * the compiled widths are 4, 8, 14, 16, 20, 32, 40, 64; the padded width is the smallest of them >= d;
  * k_scan_u serves the common case (k a power of two, no pdim filter) at every compiled width, and from nine dimensions
    on at every width up to 64 (over padded operands);
  * the chain is COMMON wherever k_scan_u serves more than eight dimensions; GENERAL where the filter is on or k is not a
    power of two, at the compiled widths 14 .. 40 only; none otherwise."""
import pytest

from chronoclust_amd import _lib

LADDER = (4, 8, 14, 16, 20, 32, 40, 64)
COMMON = dict(filter_on=False, k_pow2=True)
OUTSIDE = [dict(filter_on=True, k_pow2=True), dict(filter_on=False, k_pow2=False), dict(filter_on=True, k_pow2=False)]


def test_every_ladder_width_returns_itself_with_the_chain_it_has_today():
    # k_scan_u at every compiled width; its pruned chain beyond eight dimensions
    assert _lib.scan_width(4, **COMMON) == (4, True, "none")
    assert _lib.scan_width(8, **COMMON) == (8, True, "none")
    assert _lib.scan_width(14, **COMMON) == (14, True, "common")
    assert _lib.scan_width(16, **COMMON) == (16, True, "common")
    assert _lib.scan_width(20, **COMMON) == (20, True, "common")
    assert _lib.scan_width(32, **COMMON) == (32, True, "common")
    assert _lib.scan_width(40, **COMMON) == (40, True, "common")
    assert _lib.scan_width(64, **COMMON) == (64, True, "common")


@pytest.mark.parametrize("d,padded", [(9, 14), (13, 14), (15, 16), (17, 20), (18, 20), (19, 20), (21, 32), (31, 32),
                                       (33, 40), (39, 40), (41, 64), (63, 64)])
def test_off_ladder_widths_from_nine_dimensions_on_pad_onto_the_next_compiled_width(d, padded):
    assert _lib.scan_width(d, **COMMON) == (padded, True, "common")


def test_every_width_between_nine_and_sixty_four_has_the_common_chain():
    for d in range(9, 65):
        padded, scan_u, chain = _lib.scan_width(d, **COMMON)
        assert padded == min(w for w in LADDER if w >= d) and scan_u and chain == "common", d


@pytest.mark.parametrize("d,padded", [(3, 4), (5, 8), (6, 8), (7, 8)])
def test_up_to_eight_dimensions_an_off_ladder_width_keeps_the_lds_staged_scan(d, padded):
    assert _lib.scan_width(d, **COMMON) == (padded, False, "none")
    for kw in OUTSIDE:
        assert _lib.scan_width(d, **kw) == (padded, False, "none")


@pytest.mark.parametrize("d,padded", [(3, 4), (9, 14), (13, 14), (15, 16), (18, 20), (25, 32), (37, 40), (41, 64), (63, 64)])
def test_off_ladder_with_the_filter_on_or_k_not_a_power_of_two_has_neither(d, padded):
    for kw in OUTSIDE:
        assert _lib.scan_width(d, **kw) == (padded, False, "none"), (d, kw)


def test_ladder_widths_outside_the_common_case_keep_the_general_chain_from_14_to_40():
    for kw in OUTSIDE:
        assert _lib.scan_width(4, **kw) == (4, False, "none")
        assert _lib.scan_width(8, **kw) == (8, False, "none")
        assert _lib.scan_width(14, **kw) == (14, False, "general")
        assert _lib.scan_width(16, **kw) == (16, False, "general")
        assert _lib.scan_width(20, **kw) == (20, False, "general")
        assert _lib.scan_width(32, **kw) == (32, False, "general")
        assert _lib.scan_width(40, **kw) == (40, False, "general")
        assert _lib.scan_width(64, **kw) == (64, False, "none")  # (k_scan_p3 is compiled up to 40 dimensions)


def test_beyond_the_windowed_path_and_bad_arguments():
    # more than 64 dimensions: no window runs (k_seq_g takes the stream); the rule names the widest kernels and no fast scan
    assert _lib.scan_width(65, **COMMON) == (64, False, "none")
    assert _lib.scan_width(1024, **COMMON) == (64, False, "none")
    assert _lib.scan_width(1, **COMMON) == (4, False, "none") and _lib.scan_width(2, **COMMON) == (4, False, "none")
    for d in (0, -3, 1025):
        with pytest.raises(ValueError):
            _lib.scan_width(d, **COMMON)
