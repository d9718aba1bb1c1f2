"""The batched logit-Adam step (mst_logit_adam_init_batch / _step_batch, diff-mst_amd/csrc/mst_opt.hip) on the host simulator, through
the C ABI: every item bit for bit a single-item ``mst_logit_adam_step`` session (which tests/test_online_hostsim.py pins against
torch.optim.Adam), non-finite input confined to its item, NULL gradients, refusals.  tests/test_online_batch_gpu.py carries the same
cases (tests/online_batch_ref.py) on the device."""
import pytest

import online_batch_ref as R
import online_ref as O


@pytest.fixture()
def drv():
    from hostsim import harness

    return O.Driver(harness.lib(), "cpu")


@pytest.mark.parametrize("items", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["song3", "tails"])
def test_every_item_is_an_independent_session(drv, name, items):
    counts, _, lr, scale = O.STREAMS[name]
    R.check_equal_to_independent_sessions(drv, items, counts, 50, lr, scale)


@pytest.mark.parametrize("count", O.TAIL_COUNTS)
def test_lane_tails_and_the_loop_per_item(drv, count):
    R.check_equal_to_independent_sessions(drv, 3, (count,), 3, 1e-3, 1e-3)


@pytest.mark.parametrize("where", ["gradient", "loss"])
def test_nonfinite_input_stops_its_item_alone(drv, where):
    R.check_batch_nonfinite(drv, where)


def test_null_gradient_keeps_its_bits_for_every_item(drv):
    R.check_batch_null_gradient(drv)


def test_unsupported_arguments_launch_nothing(drv):
    R.check_batch_arguments(drv)
