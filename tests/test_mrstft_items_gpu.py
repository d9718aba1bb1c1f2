"""The per-item MR-STFT loss on the device: the checks of tests/mrstft_items_ref.py through the C ABI (every buffer the library writes
starts as NaN), and MultiResolutionSTFTLoss.per_item / pooled for what only the class does (the autograd function and its (items,)
cotangent, the value-only route, item shapes).  Shapes are small: nearly all of a case's time is the host oracle."""
import pytest
import torch

import mrstft_items_ref as ir
import mrstft_routes as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available()
    return ir.dev()


def make_loss(res, **kw):
    from mst.loss import MultiResolutionSTFTLoss

    return MultiResolutionSTFTLoss(fft_sizes=[r[0] for r in res], hop_sizes=[r[1] for r in res], win_lengths=[r[2] for r in res], **kw)


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


@pytest.mark.parametrize("items", [ir.STAGED // 10, ir.STAGED // 10 + 1], ids=["staged_640_entries", "one_item_more"])
def test_either_side_of_the_lds_staging(be, items):
    ir.check_beyond_staging(be, items)


def test_per_item_is_the_c_abi_and_differentiable(be):
    """per_item on (3, 2, n): the C ABI's values bit for bit, and backward with a (3,) cotangent is mst_mrstft_backward_items' result
    (the all-fast route: ordered writes)"""
    n = 16384
    x, y = ir.draw("class", 3, 2, n)
    g = [0.7, 1.3, 2.0]
    c = ir.Call(be, x, y, mr.R3, mr.SMOOTH)
    want, want_grad = c.forward_items(3), c.backward_items(3, g)
    f = make_loss(mr.R3, **mr.SMOOTH)
    xd = x.view(3, 2, n).to(be.device).requires_grad_(True)
    each = f.per_item(xd, y.view(3, 2, n).to(be.device))
    assert each.shape == (3,) and each.dtype == torch.float32 and each.requires_grad
    each.backward(torch.tensor(g, device=be.device))
    assert torch.equal(each.detach().cpu(), want)
    assert torch.equal(xd.grad.cpu().view(6, n), want_grad)
    # the value-only route: the same bits, nothing to differentiate
    with torch.no_grad():
        quiet = f.per_item(xd, y.view(3, 2, n).to(be.device))
    detached = f.per_item(xd.detach(), y.view(3, 2, n).to(be.device))
    assert not quiet.requires_grad and not detached.requires_grad
    assert torch.equal(quiet.cpu(), want) and torch.equal(detached.cpu(), want)


def test_pooled_is_the_loss_of_the_sections_as_one_batch(be):
    """pooled on (S, 2, n) is one item of 2 S rows: forward's value on the same tensors, bit for bit, with forward's gradient (no
    1 / items to differ by); items=2 on (2 S, 2, n) is per_item at items=2"""
    n = 16384
    x, y = ir.draw("pooled", 4, 2, n)
    f = make_loss(mr.R3, **mr.SMOOTH)
    xd, yd = x.view(4, 2, n).to(be.device), y.view(4, 2, n).to(be.device)
    a = xd[:2].clone().requires_grad_(True)
    one = f.pooled(a, yd[:2])
    one.backward(torch.ones(1, device=be.device))
    b = xd[:2].clone().requires_grad_(True)
    batch = f(b, yd[:2])
    batch.backward()
    assert one.shape == (1,) and torch.equal(one.detach().reshape(()), batch.detach())
    assert torch.equal(a.grad, b.grad)
    assert torch.equal(f.pooled(xd, yd, items=2), f.per_item(xd, yd, items=2))
    assert torch.equal(f.pooled(xd, yd, items=2)[:1], one.detach())
    with pytest.raises(ValueError, match="items"):
        f.per_item(xd, yd, items=3)
