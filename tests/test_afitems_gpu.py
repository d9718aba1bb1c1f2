"""The per-item feature loss on the MI355X: the cases of tests/test_afitems_hostsim.py (tests/online_batch_ref.py) through the C ABI of
the product library, then ``AudioFeatureLoss.per_item`` - the same bits through the package, a profile of batch size 1 broadcast, a
tensor target of equal length profiled on the way - and its errors."""
import pytest
import torch

import afprofile_ref as A
import online_batch_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def drv():
    from mst import _hip

    d = R.ItemsDriver(_hip.lib(), DEV)
    yield d
    d.scrub()  # the NaN-filled buffers and workspaces go back to the allocator as zeros


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


def test_per_item_through_the_package(drv):
    from mst.loss import AF_KEYS, AudioFeatureLoss, AudioFeatureProfile

    bs, n, m = 3, 32768, 32768
    x, prof, base, _ = R.pair(drv, bs, n, m)
    y = R.audio(bs, n, m)[1]
    f = AudioFeatureLoss(R.WEIGHTS, 44100)
    for target in (AudioFeatureProfile(prof.clone(), 44100), y.to(DEV)):  # a tensor is profiled on the way, also at equal length
        xd = x.to(DEV).requires_grad_(True)
        out = f.per_item(xd, target)
        assert tuple(out) == AF_KEYS and all(tuple(v.shape) == (bs,) and v.dtype == torch.float32 and v.is_cuda for v in out.values())
        rows = torch.stack([out[k] for k in AF_KEYS], dim=1)
        grads = torch.autograd.grad(list(out.values()), xd, [torch.ones(bs, device=DEV)] * 5)[0]
        assert torch.equal(A.bits(rows), A.bits(base["losses"])) and torch.equal(A.bits(grads), A.bits(base["grad_pred"]))
    # forward is untouched: the batch mean
    batch = f(x.to(DEV), AudioFeatureProfile(prof.clone(), 44100))
    for i, k in enumerate(AF_KEYS):
        assert abs(float(batch[k]) - float(base["losses"][:, i].double().mean())) <= R.MEAN_ULP * float(base["losses"][:, i].abs().max())
    # a profile of batch size 1 broadcasts: every item against item 0's target
    one = AudioFeatureProfile(prof[:1].clone(), 44100)
    wide = AudioFeatureProfile(prof[:1].expand(bs, -1).clone(), 44100)
    a, b = f.per_item(x.to(DEV), one), f.per_item(x.to(DEV), wide)
    assert all(torch.equal(A.bits(a[k]), A.bits(b[k])) for k in AF_KEYS)
    assert torch.equal(A.bits(a[AF_KEYS[0]][:1]), A.bits(base["losses"][:1, 0]))


def test_per_item_errors():
    from mst.loss import AudioFeatureLoss, AudioFeatureProfile

    f = AudioFeatureLoss(R.WEIGHTS, 44100)
    x = torch.zeros(3, 2, 20000, device=DEV)
    p = f.profile(torch.ones(2, 2, 17000, device=DEV))
    with pytest.raises(ValueError, match="batch size"):
        f.per_item(x, p)
    with pytest.raises(ValueError, match="batch size"):
        f.per_item(x, torch.zeros(1, 2, 17000, device=DEV))  # only a PROFILE of batch size 1 broadcasts
    with pytest.raises(ValueError, match="Hz"):
        f.per_item(x[:2], AudioFeatureProfile(p.data, 48000))
    with pytest.raises(ValueError, match="16384"):
        f.per_item(x[..., :16384], f.profile(torch.ones(3, 2, 17000, device=DEV)))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        f.per_item(x.cpu(), p)
    with pytest.raises(TypeError, match="AudioFeatureProfile"):
        f.per_item(x, None)
