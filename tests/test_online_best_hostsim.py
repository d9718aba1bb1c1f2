"""The best-iterate logit-Adam step (mst_logit_adam_step_best / _step_best_batch, diff-mst_amd/csrc/mst_opt.hip) on the host simulator,
through the C ABI: it does not perturb the fit, a hand-worked scripted sequence, ties, non-finite input, NULL gradients, every item of a
batch bit for bit a single-item session, lane tails, refusals.  tests/test_online_best_gpu.py carries the same cases
(tests/online_best_ref.py) on the device."""
import pytest

import online_best_ref as R
import online_ref as O


@pytest.fixture()
def drv():
    from hostsim import harness

    return O.Driver(harness.lib(), "cpu")


@pytest.mark.parametrize("name", ["song3", "tails"])
def test_the_fit_is_the_plain_steps(drv, name):
    R.check_does_not_perturb(drv, name)


def test_scripted_sequence(drv):
    R.check_scripted_sequence(drv)


def test_a_tie_keeps_the_earlier_iterate(drv):
    R.check_ties(drv)


@pytest.mark.parametrize("where", ["gradient", "loss"])
def test_nonfinite_input_leaves_the_best_block_alone(drv, where):
    R.check_nonfinite(drv, where)


def test_null_gradient_segment_is_in_the_snapshot(drv):
    R.check_null_gradient(drv)


@pytest.mark.parametrize("items", [3, 8])
def test_every_item_is_an_independent_best_session(drv, items):
    R.check_batch(drv, items)


@pytest.mark.parametrize("count", O.TAIL_COUNTS)
def test_lane_tails_and_the_guards_of_the_best_block(drv, count):
    R.check_lane_tails(drv, count)


def test_unsupported_arguments_launch_nothing(drv):
    R.check_refusals(drv)
