"""The per-item MR-STFT loss on the host simulator: mst_mrstft_forward_items / _backward_items (the unchanged kernel sources of
mst_stft.hip / mst_stft2.hip through the C ABI) against the scalar loss and against per-item oracles.  The checks live in
tests/mrstft_items_ref.py and run on the device as well (tests/test_mrstft_items_gpu.py); the two cases either side of the item
reduction's LDS staging take the simulator minutes and are `slow` here."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrstft_items_ref as ir  # noqa: E402
import mrstft_routes as mr  # noqa: E402


@pytest.fixture(scope="module")
def be():
    return ir.sim()


@pytest.mark.parametrize("case_id", ir.ONE_ITEM_ROUTES)
def test_one_item_is_the_scalar_loss(be, case_id):
    ir.check_one_item_is_the_scalar_loss(be, case_id)


@pytest.mark.parametrize("kw", list(ir.KWS))
@pytest.mark.parametrize("length", list(ir.LENGTHS))
@pytest.mark.parametrize("shape", ir.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_item_against_its_own_oracle(be, shape, length, kw):
    ir.check_every_item(be, shape, length, kw)


@pytest.mark.parametrize("length", list(ir.LENGTHS))
def test_an_item_touches_no_other(be, length):
    ir.check_isolation(be, length)


def test_cotangents_scale_their_own_item(be):
    ir.check_cotangents(be, "n16384_fast")


@pytest.mark.parametrize("length", list(ir.LENGTHS))
def test_mean_of_items_is_the_batch_loss(be, length):
    ir.check_mean_of_items_is_the_batch_loss(be, length)


@pytest.mark.slow
@pytest.mark.parametrize("items", [ir.STAGED // 10, ir.STAGED // 10 + 1], ids=["staged_640_entries", "one_item_more"])
def test_either_side_of_the_lds_staging(be, items):
    assert 5 * 2 * (ir.STAGED // 10) == ir.STAGED > 512  # above what the scalar reduction stages as well
    ir.check_beyond_staging(be, items)


def test_rows_that_items_does_not_divide_are_refused(be):
    """hipErrorInvalidValue (1) before any launch: the loss and the workspace stay as they were"""
    import torch
    from mst import _cabi

    x, y = ir.draw("refused", 3, 1, 3000)
    c = ir.Call(be, x, y, ir.GENERIC2, mr.SMOOTH)
    before = c.ws.clone()
    for items in (2, 4, 0, -1):
        for call in (lambda: c.forward_items(items), lambda: c.forward_items(items, keep=False),
                     lambda: c.backward_items(items, [1.0] * max(items, 1))):
            with pytest.raises(_cabi.AbiError) as e:
                call()
            assert e.value.code == 1
    assert torch.equal(c.ws.view(torch.int32), before.view(torch.int32))


def test_the_value_only_forward_has_the_same_bits(be):
    x, y = ir.draw("eval", 3, 2, 16384)
    c = ir.Call(be, x, y, mr.R3, mr.SMOOTH)
    kept = c.forward_items(3)
    c.fresh()
    assert ir.same_bits(c.forward_items(3, keep=False), kept)
