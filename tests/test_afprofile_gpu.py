"""Feature profiles of AudioFeatureLoss on the MI355X: the cases of tests/afprofile_ref.py through the C ABI of the product library and
through the package (``AudioFeatureLoss.profile`` / ``forward`` with a profile or a target of another length), at the reference's
sizes; then ``mst.online.optimize`` against a reference mix of another length, and against its stored profile."""
import pytest
import torch

import afprofile_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class PackageDriver:
    """The interface of ``afprofile_ref.Driver`` on the package's own classes: what a user calls."""

    device = torch.device(DEV)

    def check_guards(self):
        pass

    def profile(self, x):
        from mst.loss import AudioFeatureLoss

        p = AudioFeatureLoss(R.AF_WEIGHTS, 44100).profile(x.to(DEV))
        assert p.n_samples == x.shape[-1] and p.sample_rate == 44100 and p.data.is_cuda and not p.data.requires_grad
        return p.data

    def loss(self, pred, profile, weights, grad_losses=None):
        from mst.loss import AF_KEYS, AudioFeatureLoss, AudioFeatureProfile

        xd = pred.to(DEV).requires_grad_(grad_losses is not None)
        ld = AudioFeatureLoss(weights, 44100)(xd, AudioFeatureProfile(profile, 44100))
        assert tuple(ld) == AF_KEYS and all(v.dim() == 0 for v in ld.values())
        vals = torch.stack([ld[k] for k in AF_KEYS])
        out = dict(losses=vals.detach().cpu())
        if grad_losses is not None:
            (vals * torch.tensor(grad_losses, device=DEV)).sum().backward()
            out["grad_pred"] = xd.grad.cpu()
        return out


@pytest.fixture(scope="module")
def cabi():
    from mst import _hip

    return R.Driver(_hip.lib(), DEV)


@pytest.fixture(params=["cabi", "package"])
def drv(request, cabi):
    return cabi if request.param == "cabi" else PackageDriver()


# ---- cases 1-7 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,n_pred,n_target", [(1, 16385, 50001), (3, 50001, 16385), (2, 131072, 40000), (1, 16385, 131072),
                                                (2, 40000, 40000)])
def test_unequal_lengths_three_way(drv, bs, n_pred, n_target, record):
    R.check_three_way(drv, bs, n_pred, n_target, record)


def test_profile_views_against_the_reference_functions(drv, record):
    R.check_golden_features(drv, record)


@pytest.mark.parametrize("fixture", ["af_loss.npz", "af_loss_unequal.npz"])
def test_loss_against_the_reference_class(drv, fixture, record):
    R.check_golden_loss(drv, fixture, record)


def test_known_answers(drv):
    R.check_known_answers(drv)


def test_long_signal(cabi, record):
    R.check_long(cabi, record=record)


@pytest.mark.parametrize("bs,n_pred,n_target", [(3, 50001, 16385), (8, 32768, 20000)])  # the plain walk and the per-XCD walk (bs % 8 == 0)
def test_determinism_and_bounds_of_writes(cabi, bs, n_pred, n_target):
    R.check_determinism_and_bounds(cabi, bs, n_pred, n_target)


def test_validation(cabi):
    R.check_validation(cabi)


def test_a_target_of_another_length_is_profiled(cabi):
    """forward(input, tensor of another length) = forward(input, profile(tensor)) = the C ABI's bits; the profile carries no graph."""
    from mst.loss import AF_KEYS, AudioFeatureLoss

    x, y = R.signals(3, 50001, 16385)
    f = AudioFeatureLoss(R.AF_WEIGHTS, 44100)
    got = []
    for target in (y.to(DEV).requires_grad_(True), f.profile(y.to(DEV))):
        xd = x.to(DEV).requires_grad_(True)
        ld = f(xd, target)
        vals = torch.stack([ld[k] for k in AF_KEYS])
        (vals * torch.tensor(R.COTANGENT, device=DEV)).sum().backward()
        got.append((vals.detach(), xd.grad))
        assert not isinstance(target, torch.Tensor) or target.grad is None  # the target side never receives a gradient
    ref = cabi.loss(x, cabi.profile(y), R.AF_WEIGHTS, R.COTANGENT)
    for vals, grad in got:
        assert torch.equal(R.bits(vals), R.bits(ref["losses"])) and torch.equal(R.bits(grad), R.bits(ref["grad_pred"]))
    with torch.no_grad():  # a value-only call
        z = f(x.to(DEV), y.to(DEV))
    assert torch.equal(R.bits(torch.stack([z[k] for k in AF_KEYS])), R.bits(ref["losses"]))
    moved = f.profile(y.to(DEV)).to("cpu")
    assert not moved.data.is_cuda and moved.n_samples == 16385 and tuple(moved.barkspectrum.shape) == (3, 24, 2)
    assert AudioFeatureLoss.Profile is type(moved)


def test_python_validation():
    from mst.loss import AudioFeatureLoss, AudioFeatureProfile

    f = AudioFeatureLoss(R.AF_WEIGHTS, 44100)
    x = torch.zeros(2, 2, 20000, device=DEV)
    p = f.profile(torch.ones(2, 2, 17000, device=DEV))
    with pytest.raises(ValueError, match="batch size"):
        f(x, torch.zeros(3, 2, 17000, device=DEV))
    with pytest.raises(ValueError, match="batch size"):
        f(x[:1], p)
    with pytest.raises(ValueError, match="Hz"):
        f(x, AudioFeatureProfile(p.data, 48000))
    with pytest.raises(ValueError):
        f(x, torch.zeros(2, 1, 17000, device=DEV))  # a target that is not stereo
    with pytest.raises(ValueError):
        f(x, torch.zeros(2, 17000, device=DEV))
    with pytest.raises(ValueError):
        f(torch.zeros(2, 1, 20000, device=DEV), p)
    with pytest.raises(ValueError, match="16384"):
        f(x, torch.zeros(2, 2, 16384, device=DEV))
    with pytest.raises(ValueError, match="16384"):
        f.profile(torch.zeros(1, 2, 16384, device=DEV))
    with pytest.raises(ValueError, match="16384"):
        f(x[..., :16384], p)
    for bad in (lambda: f.profile(torch.zeros(1, 2, 20000)), lambda: f(x, torch.zeros(2, 2, 17000)), lambda: f(x, p.to("cpu")),
                lambda: f(x.cpu(), p)):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            bad()
    for target in (None, torch.zeros(2, 2, 17000).numpy(), p.data.tolist()):  # neither a tensor nor a profile
        with pytest.raises(TypeError, match="AudioFeatureProfile"):
            f(x, target)


# ---- case 8: optimize() against a reference of another length -----------------------------------------------------------------------------
ITERS, LR, SEEDS, M = 20, 1e-3, (0, 1, 2), 49152


def other_song(seed):
    """tracks (T, N) of tests/test_online_gpu.py and a reference mix (2, M): the console's output for parameters from [0.25, 0.75] on
    an M-sample draw of the same coloured noise."""
    import test_online_gpu as O

    return O.song(seed)[0], O.song(seed, O.T, M)[1]


def optimise(seed, ref, n_iters=ITERS, loss=None, console=None):
    import test_online_gpu as O
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize

    torch.manual_seed(seed)
    return optimize(other_song(seed)[0], ref, console or AdvancedMixConsole(44100), loss or AudioFeatureLoss(O.WEIGHTS, 44100),
                    n_iters=n_iters, lr=LR)


@pytest.mark.parametrize("seed", SEEDS)
def test_descent_towards_a_reference_of_another_length(seed, record):
    history = optimise(seed, other_song(seed)[1])[7]["loss"]
    print(f"\n[optimize seed {seed}, reference of {M} samples] loss {history[0]:.4e} -> {history[-1]:.4e} (ratio {history[-1] / history[0]:.3f})")
    record(first=history[0], last=history[-1])
    assert len(history) == ITERS
    # measured 0.305 / 0.154 / 0.237 on the MI355X (the equal-length test of tests/test_online_gpu.py: 0.286 / 0.142 / 0.231 against
    # the same 0.8), so its bound is adopted
    assert history[-1] < 0.8 * history[0]


def test_a_stored_profile_is_the_tensor_reference():
    import test_online_gpu as O
    from mst.loss import AudioFeatureLoss, AudioFeatureProfile

    ref = other_song(0)[1]
    stored = AudioFeatureLoss(O.WEIGHTS, 44100).profile(ref[None]).data.cpu()  # as a saved profile comes back
    a, b = optimise(0, ref), optimise(0, AudioFeatureProfile(stored, 44100).to(DEV))
    assert O.same_bits(a[0], b[0]) and a[7] == b[7]
    for i in (1, 3, 5):
        assert O.same_bits(a[i], b[i])
    with pytest.raises(ValueError, match="batch size 1"):
        optimise(0, AudioFeatureProfile(torch.cat([stored, stored]), 44100).to(DEV), n_iters=1)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        optimise(0, AudioFeatureProfile(stored, 44100), n_iters=1)
    with pytest.raises(ValueError):
        optimise(0, ref[:1], n_iters=1)
    with pytest.raises(TypeError, match="AudioFeatureProfile"):
        optimise(0, ref.cpu().numpy(), n_iters=1)


def test_the_reference_is_profiled_once():
    import test_online_gpu as O
    from mst.loss import AudioFeatureLoss

    loss, calls = AudioFeatureLoss(O.WEIGHTS, 44100), []
    inner = loss.profile

    def counting(x):
        calls.append(tuple(x.shape))
        return inner(x)

    loss.profile = counting
    optimise(0, other_song(0)[1], n_iters=5, loss=loss)
    assert calls == [(1, 2, M)]
    optimise(0, O.song(0)[1], n_iters=2, loss=loss)  # an equal-length tensor keeps the paired path: no profile at all
    assert len(calls) == 1

    seen = []

    def plain(mix, target):  # a loss function without a profile method is handed the tensor and decides
        seen.append(tuple(target.shape))
        return mix.pow(2).mean()

    optimise(0, other_song(0)[1], n_iters=2, loss=plain)
    assert seen == [(1, 2, M)] * 2


def test_no_host_wait_inside_the_loop():
    import test_online_gpu as O
    from mst import online
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole

    tracks, ref = other_song(0)
    console, loss = AdvancedMixConsole(44100, validate="deferred"), AudioFeatureLoss(O.WEIGHTS, 44100)
    online.optimize(tracks, ref, console, loss, n_iters=1)  # the constant tables of console and loss are built on their first call
    torch.manual_seed(0)
    r = online._Run(tracks, ref, console, loss, 0.001, LR, ITERS, (0.9, 0.999), 1e-8, None, None, {})  # the profile is taken here
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for n in range(ITERS):
            r.iterate(n)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    history = r.finish()[7]["loss"]
    console.check_parameters()
    assert len(history) == ITERS and history[-1] < 0.8 * history[0]  # and the loop did its work
