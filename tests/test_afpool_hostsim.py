"""The pooled feature loss (mst_af_profile_pooled / mst_afloss_forward_profile_pooled / _backward_profile_pooled,
diff-mst_amd/csrc/mst_af.hip) on the host simulator, through the C ABI, at n = 17000 (three frames).  tests/test_afpool_gpu.py carries
the same cases (tests/online_sections_ref.py) on the device at n = 32768 and the ragged n = 40962, and those a simulated transform of
1.8 s per signal row makes too slow for this file: three sections three-way, four copies, isolation, the exact zero, the second run."""
import pytest

import online_sections_ref as P

N, M = 17000, 17500


@pytest.fixture()
def drv():
    from hostsim import harness

    return P.PoolDriver(harness.lib(), "cpu")


def test_one_section_is_the_per_item_call(drv):
    P.check_one_section_is_the_items_call(drv, N, M)


def test_pooled_three_way(drv):
    P.check_pooled_three_way(drv, 2, 2, N, M)  # three sections of one item: the golden case below here, three-way on the device


def test_copies_of_one_section(drv):
    P.check_copies(drv, N, M, copies=(2,))  # four copies: on the device


def test_golden_features_of_three_sections(drv):
    P.check_golden(drv)


def test_known_answers(drv):
    P.check_known_answers(drv, N, noise=False, zero=False)  # the exact zero against the own profile: on the device


def test_unsupported_arguments_launch_nothing(drv):
    P.check_pooled_refusals(drv)
