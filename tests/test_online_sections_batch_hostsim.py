"""A batch of sectioned fits on the host simulator: the step for ``items`` parameter sets with ``sections`` gradient rows each
(mst_logit_adam_init_sections_batch / _step_sections_batch, diff-mst_amd/csrc/mst_opt.hip) through the C ABI, and
``AudioFeatureLoss.pooled(..., items=B)`` / ``profile(..., pool=True, items=B)`` on the simulator's library.
tests/test_online_sections_batch_gpu.py carries the same cases (tests/online_sections_batch_ref.py) on the device."""
import pytest

import online_ref as O
import online_sections_batch_ref as Q


@pytest.fixture()
def drv():
    from hostsim import harness

    return O.Driver(harness.lib(), "cpu")


@pytest.fixture()
def loss():
    from hostsim import harness

    with Q.SimLoss(harness.lib()) as loss:
        yield loss


# ---- the step ---------------------------------------------------------------------------------------------------------------------------
# The simulator takes 10 - 25 ms per launch, so the lane-tail counts run the three steps that tests/online_ref.py gives their streams
# (a wrong lane shows in the first step and a difference never heals); the device file runs them for 50 like the rest.
@pytest.mark.parametrize("best", [False, True])
@pytest.mark.parametrize("counts", [Q.COUNTS] + [(c,) for c in O.TAIL_COUNTS])
def test_one_item_is_the_sections_call(drv, counts, best):
    Q.check_one_item_is_the_sections_call(drv, counts, best, steps=Q.STEPS if counts == Q.COUNTS else 3)


@pytest.mark.parametrize("best", [False, True])
def test_one_section_is_the_batch_call(drv, best):
    Q.check_one_section_is_the_batch_call(drv, 3, best)


# every value of items {2, 3, 5} and of sections {2, 3, 8}; the device file runs all nine combinations
@pytest.mark.parametrize("items,sections", [(2, 2), (3, 3), (5, 8)])
def test_every_item_is_an_independent_sections_session(drv, items, sections):
    Q.check_items_of_sections(drv, items, sections, with_sum=items == 2)


@pytest.mark.parametrize("count", O.TAIL_COUNTS)
def test_lane_tails_and_the_loop_per_item(drv, count):
    Q.check_items_of_sections(drv, 3, 3, counts=(count,), steps=3, best=True, with_sum=False)


@pytest.mark.parametrize("where", ["nan", "overflow"])
def test_nonfinite_addend_or_sum_stops_its_item_alone(drv, where):
    Q.check_nonfinite_item(drv, where)


def test_null_gradient_keeps_its_bits_for_every_item_and_row(drv):
    Q.check_null_gradient(drv)


def test_scripted_losses_settle_every_item_on_its_own(drv):
    Q.check_scripted_sequences(drv)


def test_unsupported_arguments_launch_nothing(drv):
    Q.check_refusals(drv)


# ---- the loss surface: n = 17000, items = 2, S = 2 ----------------------------------------------------------------------------------------
# The simulator transforms a signal row in about 2 s: one shared call at four rows for the three-way bound, one more for the isolation,
# the five terms at items = 1.  The gradient at items = 1, the broadcast profile, the exact zero and the second run are device cases.
N, M = 17000, 20000


def test_items_one_is_todays_pooled(loss):
    Q.check_items_one_is_todays_call(loss, "cpu", N, M, thorough=False)


def test_pooled_items_three_way(loss):
    Q.check_pooled_three_way(loss, "cpu", 2, 2, N, M, second_run=False)


def test_items_are_isolated(loss):
    Q.check_isolation(loss, "cpu", 2, 2, N, M, separately=False)


def test_loss_refusals(loss):
    Q.check_loss_refusals(loss, "cpu")
