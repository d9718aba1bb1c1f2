"""The section-summing logit-Adam step (mst_logit_adam_init_sections / _step_sections, diff-mst_amd/csrc/mst_opt.hip) on the host
simulator, through the C ABI: one section bit for bit the single step (with and without a best block), several sections bit for bit
a single session fed the host's fp32 sum, non-finite addends and sums, NULL gradients, refusals, the best block.
tests/test_online_sections_gpu.py carries the same cases (tests/online_sections_ref.py) on the device."""
import pytest

import online_ref as O
import online_sections_ref as P


@pytest.fixture()
def drv():
    from hostsim import harness

    return O.Driver(harness.lib(), "cpu")


@pytest.mark.parametrize("best", [False, True])
@pytest.mark.parametrize("name", ["song3", "tails"])
def test_one_section_is_the_single_step(drv, name, best):
    P.check_one_section_is_the_single_step(drv, name, best)


@pytest.mark.parametrize("sections", [2, 3, 8])
def test_sections_are_summed_in_order(drv, sections):
    counts, _, lr, scale = O.STREAMS["song3"]
    P.check_sum_of_sections(drv, sections, counts, 20, lr, scale)


@pytest.mark.parametrize("count", O.TAIL_COUNTS)
def test_lane_tails_and_the_loop(drv, count):
    P.check_sum_of_sections(drv, 3, (count,), 3, 1e-3, 1e-3)


@pytest.mark.parametrize("where", ["nan", "overflow"])
def test_nonfinite_addend_or_sum_stops_the_step(drv, where):
    P.check_sections_nonfinite(drv, where)


def test_null_gradient_keeps_its_bits_in_every_row(drv):
    P.check_sections_null_gradient(drv)


def test_unsupported_arguments_launch_nothing(drv):
    P.check_sections_refusals(drv)


def test_best_block_gives_the_single_kernels_verdicts(drv):
    P.check_sections_best(drv)
