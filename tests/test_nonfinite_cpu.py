"""The CPU oracle on the non-finite data set of tests/nonfinite_cases.py:
the same tables and plans as tests/test_nonfinite_routes.py, against the same
numpy reference, so the oracle and the contract the GPU routes are held to
cannot drift apart (single-threaded accumulate and the thread merge)."""
import pytest

from tests import nonfinite_cases as nc

CASES = dict(nc.SUM_CASES, **nc.MM_CASES)


@pytest.fixture(scope="module")
def tables():
    return {}


def table_of(tables, kind):
    if kind not in tables:
        tables[kind] = nc.oracle_table(nc.data(kind))
    return tables[kind]


@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("table", ["clean", "interp"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_case(tables, case, table, nthreads):
    got = nc.oracle_groups(table_of(tables, table), CASES[case], nthreads)
    nc.assert_same_groups(got, nc.reference(nc.data(table), CASES[case]))


@pytest.mark.parametrize("table", ["clean_del", "interp_del"])
@pytest.mark.parametrize("case", nc.DEL_CASES)
def test_oracle_deleted_specials(tables, case, table):
    got = nc.oracle_groups(table_of(tables, table), CASES[case])
    nc.assert_same_groups(got, nc.reference(nc.data(table), CASES[case]))


@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("case", ["radix", "radix_mm"])
def test_oracle_radix_table(tables, case, nthreads):
    spec = nc.RADIX_CASE if case == "radix" else nc.RADIX_MM_CASE
    got = nc.oracle_groups(table_of(tables, "radix"), spec, nthreads)
    nc.assert_same_groups(got, nc.reference(nc.data("radix"), spec))
