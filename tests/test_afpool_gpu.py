"""The pooled feature loss on the MI355X: the cases of tests/test_afpool_hostsim.py (tests/online_sections_ref.py) through the C ABI of
the product library, at n = 32768 and the ragged n = 40962 (the tail loads of k_af_stats / k_af_bwd_gather), with 1, 2, 3 and 4
sections."""
import pytest

import online_sections_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENGTHS = [(32768, 40000), (40962, 33000)]  # (sections, reference)


@pytest.fixture()
def drv():
    from mst import _hip

    d = P.PoolDriver(_hip.lib(), DEV)
    yield d
    d.scrub()


@pytest.mark.parametrize("n,m", LENGTHS)
def test_one_section_is_the_per_item_call(drv, n, m):
    P.check_one_section_is_the_items_call(drv, n, m)


@pytest.mark.parametrize("n,m", LENGTHS)
@pytest.mark.parametrize("items,sections", [(1, 3), (2, 2)])
def test_pooled_three_way(drv, items, sections, n, m, record):
    P.check_pooled_three_way(drv, items, sections, n, m, record)


@pytest.mark.parametrize("n,m", LENGTHS)
def test_copies_of_one_section(drv, n, m):
    P.check_copies(drv, n, m)


def test_golden_features_of_three_sections(drv, record):
    P.check_golden(drv, record)


def test_known_answers(drv):
    P.check_known_answers(drv, 40962)


@pytest.mark.parametrize("n,m", LENGTHS)
def test_nan_stays_in_its_item(drv, n, m):
    P.check_isolation(drv, n, m)


@pytest.mark.parametrize("items,sections,n,m", [(1, 3, 40962, 33000), (2, 2, 32768, 40000), (1, 4, 40962, 33000)])
def test_two_runs_are_bit_equal_between_untouched_guards(drv, items, sections, n, m):
    P.check_reproducible(drv, items, sections, n, m)


def test_unsupported_arguments_launch_nothing(drv):
    P.check_pooled_refusals(drv)
