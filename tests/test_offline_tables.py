"""The offline PreDeCon phase (cc_offline: K5 core flags, K6 eps-neighbour bitmask, K7 subspace preference, K8 weighted
reachability, the neighbour lists, the ordered expansion, k_cluster_merge) against the CPU oracle on injected tables
(tests/table_util.py): chains that span the bitmask, a dense table, lattice tables that sit on the three thresholds,
mixed tables with every reason for a pcore not to be core, a shifted and scaled table - at sizes around one 64-bit word,
one batch of 64 words (4 096 rows) and the default sharding threshold (8 192), at every compiled width of
k_eps_neighbours and its neighbours, and at 32 768 x 40 (the fall-back from the 50 000 x 40 of the stress configuration).  The same tables
then run row-sharded in in-process groups of 2, 3 and 8 ranks, every rank against the oracle.

Everything is compared for bit equality: core, pdim, nn, nw per pcore, num_core, the clusters' members in merge order
and their w, cf1, cf2, cen, pref.  Each table first proves on the oracle's own output that the structure it exists for
is there (table_util.check_structure)."""
import time

import pytest

import table_util as T

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

LARGEST = "chains-32768x40"
NAMES = [n for n in T.OFFLINE_TABLES if n != LARGEST]
# in groups of 8, some ranks own no rows of the small tables (blocks of whole 64-row words)
WORLDS = (2, 3, 8)

_cases = {}


def _case(name):
    """(table, params, oracle result) of a table, the structure check done; the oracle runs once per table."""
    if name not in _cases:
        t, par, meta = T.build_table(name)
        t0 = time.time()
        exp = T.oracle_offline(T.make_oracle(par, t))
        print("%s: oracle %.1f s" % (name, time.time() - t0))
        T.check_structure(t, par, meta, *exp)
        _cases[name] = (t, par, exp)
    return _cases[name]


def _single(t, par):
    from chronoclust_amd import _lib
    h = _lib.Handle(0)
    try:
        return T.handle_offline(T.fill_handle(h, par, t))
    finally:
        h.close()


@pytest.mark.parametrize("name", NAMES)
def test_offline_table_against_oracle(name):
    t, par, exp = _case(name)
    T.same_offline(_single(t, par), exp, name)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", NAMES)
def test_offline_table_sharded_against_oracle(name, world):
    """p rows split over the ranks in blocks of whole words, three all-gathers; every rank against the oracle."""
    t, par, exp = _case(name)
    for rank, got in enumerate(T.group_offline(world, par, t)):
        T.same_offline(got, exp, "%s rank %d of %d" % (name, rank, world))


def test_offline_repeated_on_one_handle():
    """A handle's buffers are reused from call to call: a large table, then a small one, then the large one again
    (scratch sized by the larger table, stale words beyond the smaller one's)."""
    from chronoclust_amd import _lib
    h = _lib.Handle(0)
    for name in ("chains-4097x16", "mixed-k4-65x4", "ties-300x3", "chains-4097x16"):
        t, par, exp = _case(name)
        h.reset()
        T.same_offline(T.handle_offline(T.fill_handle(h, par, t)), exp, name)
    h.close()


@pytest.mark.timeout(200)
def test_offline_largest_table_against_oracle():
    """Chains of 300 in 32 768 pcores of 40 dimensions: one GPU, then two ranks.  The table of the stress configuration
    (50 000 x 40) was tried first: the oracle's offline phase on it took 311 s on the GPU machine's CPU (149 s on a
    build machine), above the five minutes allowed for it, so this is the fall-back size; here the oracle takes
    66 s there (65 s on a build machine; the whole test 67 s), and the time limit is three times that."""
    t, par, exp = _case(LARGEST)
    T.same_offline(_single(t, par), exp, LARGEST)
    for rank, got in enumerate(T.group_offline(2, par, t)):
        T.same_offline(got, exp, "%s rank %d of 2" % (LARGEST, rank))
