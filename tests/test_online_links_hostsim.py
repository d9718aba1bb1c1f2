"""Linked rows on the host simulator: the step in which rows of the track segment share one set of logits and a follower carries the
mirrored pan (mst_logit_adam_init_linked / _step_linked, diff-mst_amd/csrc/mst_opt.hip) through the C ABI.
tests/test_online_links_gpu.py carries the same cases (tests/online_links_ref.py) on the device."""
import pytest

import online_links_ref as K
import online_ref as O


@pytest.fixture()
def drv():
    from hostsim import harness

    return O.Driver(harness.lib(), "cpu")


# The simulator takes 10 - 25 ms per launch: the streams run three steps here (a wrong lane or a wrong sum shows in the first step
# and a difference never heals) and 50 on the device.
STEPS = 3


@pytest.mark.parametrize("best", [False, True])
@pytest.mark.parametrize("rows", [3, 10])
@pytest.mark.parametrize("items,sections", [(1, 1), (2, 2), (3, 3)])
def test_identity_map_is_the_sections_batch_call(drv, items, sections, rows, best):
    K.check_identity_is_sections_batch(drv, items, sections, rows, best, steps=STEPS)


@pytest.mark.parametrize("sections", [1, 3])
@pytest.mark.parametrize("name", sorted(K.MAPS))
def test_linked_step_matches_adam_on_the_leader_rows(drv, name, sections):
    K.check_parity(drv, name, sections, STEPS)


def test_zero_logits_pan_both_channels_to_the_centre(drv):
    K.check_zero_logits_pan_centre(drv)


@pytest.mark.parametrize("where", ["nan", "overflow"])
def test_nonfinite_follower_or_group_sum_stops_its_item_alone(drv, where):
    K.check_nonfinite_follower(drv, where)


@pytest.mark.parametrize("which", [0, 1])
def test_null_gradient_segment_keeps_its_bits(drv, which):
    K.check_null_gradient(drv, which)


def test_best_snapshot_is_the_iterate_before_the_update_for_every_member(drv):
    K.check_best_snapshot(drv)


@pytest.mark.parametrize("best", [False, True])
def test_every_item_is_a_single_item_linked_session(drv, best):
    K.check_items_are_single_sessions(drv, best, steps=STEPS)


def test_unsupported_arguments_launch_nothing(drv):
    K.check_refusals(drv)
