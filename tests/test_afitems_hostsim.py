"""The per-item feature loss (mst_afloss_forward_profile_items / _backward_profile_items, diff-mst_amd/csrc/mst_af.hip) on the host
simulator, through the C ABI: every item a batch of one beside the batch calls it shares its analysis with.  Five and six frames per
signal (32768 samples, and 40962 with a ragged tail), targets of 32768 and 49152 samples; tests/test_afitems_gpu.py carries the same
cases (tests/online_batch_ref.py) on the device."""
import pytest

import online_batch_ref as R


@pytest.fixture(scope="module")
def drv():
    from hostsim import harness

    return R.ItemsDriver(harness.lib(), "cpu")


@pytest.mark.parametrize("n,m", [(32768, 49152), (40962, 32768)])
def test_a_batch_of_one_is_the_batch_call(drv, n, m):
    R.check_batch_of_one(drv, n, m)


@pytest.mark.parametrize("bs,n,m", [(2, 40962, 32768), (3, 32768, 32768), (4, 32768, 49152)])
def test_mean_over_items_is_the_batch_value(drv, bs, n, m):
    R.check_mean_over_items(drv, bs, n, m)


@pytest.mark.parametrize("bs,n,m", [(2, 40962, 32768), (4, 32768, 49152)])
def test_gradient_is_exactly_bs_times_the_batch_gradient(drv, bs, n, m):
    R.check_scaling(drv, bs, n, m)


def test_items_three_way_against_the_oracle(drv, record):
    R.check_items_three_way(drv, 3, 40962, 49152, record)


def test_items_are_isolated(drv):
    R.check_isolation(drv, 3, 32768, 32768)


def test_reproducible_guarded_and_refusing(drv):
    R.check_reproducible_and_refusals(drv, 3, 32768, 32768)
