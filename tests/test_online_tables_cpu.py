"""The injected tables of tests/test_online_tables.py against the CPU oracle alone (no GPU): every generator of
table_util.ONLINE_TABLES builds its case, the oracle runs the online phase on it, and `check_online` asserts that the
structure the case exists for is there - the foreign row wins every victim point, every path occurs on the stale tables
and an outlier is promoted at w == beta mu, the lattice tables hold exact ties and radii on the threshold."""
import pytest

import table_util as T


@pytest.mark.parametrize("name", list(T.ONLINE_TABLES))
def test_online_table_structure(name):
    case = T.build_online(name)
    T.check_online(case, T.oracle_online(case))
