"""Batched fits on the MI355X: the cases of tests/test_online_batch_hostsim.py on the device (through the C ABI of the product library,
tests/online_batch_ref.py), then ``mst.online.optimize_batch`` end to end - B = 1 beside ``optimize``, three songs against three
references of another length, one song against a profile of batch 3, no host wait inside the loop, ``pick`` into ``render_blocks`` - and
the errors.  Songs, references and the replay bound are those of tests/test_online_gpu.py and tests/test_afprofile_gpu.py."""
import functools

import pytest
import torch

import afprofile_ref as A
import online_batch_ref as R
import online_ref as O
from oracle import loss_restated as ol

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, M = 1e-3, 49152
AF_KEYS = ol.AF_KEYS


@pytest.fixture()
def drv():
    from mst import _hip

    d = O.Driver(_hip.lib(), DEV)
    yield d
    R.scrub(d)  # the NaN-filled buffers go back to the allocator as zeros


# ---- the kernels through the C ABI: the simulator's cases -----------------------------------------------------------------------
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


# ---- optimize_batch() end to end --------------------------------------------------------------------------------------------------
def songs(seeds):
    """tracks (B, T, N) of tests/test_online_gpu.py's songs and their references of M samples (B, 2, M), on the device."""
    import test_online_gpu as G

    return torch.stack([G.song(s)[0] for s in seeds]), torch.stack([G.song(s, G.T, M)[1] for s in seeds])


def fit(tracks, ref, n_iters, seed=0, capture=True, callback=None, **kw):
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_batch

    console = AdvancedMixConsole(44100)
    cap = callback if callback is not None else (G.Capture() if capture else None)
    torch.manual_seed(seed)
    out = optimize_batch(tracks, ref, console, AudioFeatureLoss(G.WEIGHTS, 44100), n_iters=n_iters, lr=LR, callback=cap, **kw)
    return out, cap, console


def assert_replay(tag, cap, final_logits, b, record=None):
    """Item b's logits after every step against the float64 recurrence on its captured gradients, with tests/test_online_gpu.py's bound."""
    assert [g is None for g in cap.grads[0]] == [False, True, False]  # use_fx_bus=False: the fx parameters have no gradient
    theta0 = [t[b].cpu().reshape(-1) for t in cap.logits[0]]
    after = [[t[b] for t in logits] for logits in cap.logits[1:]] + [[t[b] for t in final_logits]]
    for k, got in enumerate(after, start=1):
        stream = [None if cap.grads[0][s] is None else torch.stack([g[s][b].cpu().reshape(-1) for g in cap.grads[:k]]) for s in range(3)]
        t64 = O.adam_f64(theta0, stream, LR)
        e_torch = O.e_stat(O.adam_torch(theta0, stream, LR), t64, theta0)
        e_kernel, floor = O.e_stat(got, t64, theta0), O.floor_term(t64, theta0)
        print(f"[replay {tag} item {b} step {k}] e(kernel) = {e_kernel:.3e}, e(torch fp32) = {e_torch:.3e}, floor {floor:.3e}")
        if record is not None:
            record(**{f"item{b}_step{k}": (e_kernel, e_torch, floor)})
        assert e_kernel <= O.SLACK * e_torch + floor
        assert G_same(got[1].cpu().reshape(-1), theta0[1])  # no gradient: the fx logits are the start point's


def G_same(a, b):
    return a.shape == b.shape and torch.equal(O.bits(a), O.bits(b))


def test_a_batch_of_one_beside_optimize(record):
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize, pick

    tracks, ref = G.song(0)
    (out, cap, console) = fit(tracks[None], ref[None], 3)
    single_cap = G.Capture()
    torch.manual_seed(0)
    single = optimize(tracks, ref, AdvancedMixConsole(44100), AudioFeatureLoss(G.WEIGHTS, 44100), n_iters=3, lr=LR, callback=single_cap)
    assert len(out) == 9 and out[8] == [None]
    for a, b in zip(cap.logits[0], single_cap.logits[0]):
        assert G_same(a, b)  # the same start point
    # the first iteration's terms: both routes against the float64 oracle on the mix they saw, afprofile_ref's three-way bound
    with torch.no_grad():
        mix = console(tracks[None], *cap.params[0], use_fx_bus=False)[1].cpu()
    v64 = ol.audio_feature_loss(mix.double(), ref[None].cpu().double(), G.WEIGHTS)
    v32 = ol.audio_feature_loss(mix, ref[None].cpu(), G.WEIGHTS)
    for k in AF_KEYS:
        t64 = float(v64[k])
        err32 = abs(float(v32[k]) - t64) / abs(t64)
        e_batch, e_single = abs(float(cap.losses[0][k][0]) - t64) / abs(t64), abs(float(single_cap.losses[0][k]) - t64) / abs(t64)
        print(f"[B = 1, {k}] batch {e_batch:.2e} single {e_single:.2e} fp32 oracle {err32:.2e}")
        record(**{k.replace("-", "_"): (e_batch, e_single, err32)})
        assert e_batch <= 3 * err32 + 2e-5 and e_single <= 3 * err32 + 2e-5
        assert tuple(out[7][k].shape) == (3, 1) and float(out[7][k][0, 0]) == float(cap.losses[0][k][0])
    assert_replay("B = 1", cap, (out[1], out[3], out[5]), 0, record)
    one = pick(out, 0)
    assert [tuple(one[i].shape) for i in (0, 1, 3, 5)] == [tuple(single[i].shape) for i in (0, 1, 3, 5)]
    assert list(one[7]) == list(single[7]) and all(len(v) == 3 for v in one[7].values())


@functools.lru_cache(maxsize=None)
def three_songs():
    """One captured run of three songs against three references of another length, shared by the cases below and never modified."""
    tracks, ref = songs((0, 1, 2))
    return fit(tracks, ref, 5) + (tracks,)


def test_three_songs_replay_and_descent(record):
    out, cap, _, _ = three_songs()
    assert out[8] == [None] * 3
    assert [tuple(t.shape) for t in (out[0], out[1], out[3], out[5])] == [(3, 2, 32768), (3, 3, 27), (3, 25), (3, 26)]
    history = out[7]
    assert list(history) == ["loss"] + list(AF_KEYS)
    for name, h in history.items():
        assert tuple(h.shape) == (5, 3) and not h.is_cuda and bool(torch.isfinite(h).all()), name
    for b in range(3):
        assert_replay("three songs", cap, (out[1], out[3], out[5]), b, record)
        first, last = float(history["loss"][0, b]), float(history["loss"][-1, b])
        print(f"[three songs item {b}] loss {first:.4e} -> {last:.4e}")
        record(**{f"item{b}_loss": (first, last)})
        assert last < first
    # the history is the captured terms and their left-to-right fp32 sum, per item
    for k, losses in enumerate(cap.losses):
        total = torch.zeros(3, device=DEV)
        for name in AF_KEYS:
            total = total + losses[name]
            assert torch.equal(history[name][k], losses[name].cpu())
        assert torch.equal(history["loss"][k], total.cpu())


def test_pick_feeds_render_blocks():
    from mst.online import pick, render_blocks

    out, cap, console, tracks = three_songs()
    for b in range(3):
        one = pick(out, b)
        assert len(one) == 8 and G_same(one[0], out[0][b])
        assert [tuple(one[i].shape) for i in (1, 3, 5)] == [(1, 3, 27), (1, 25), (1, 26)]
        assert one[7]["loss"] == out[7]["loss"][:, b].tolist()
        full = render_blocks(tracks[b], one[1], one[3], one[5], console, block_size=32768)
        assert tuple(full.shape) == (2, 32768) and bool(torch.isfinite(full).all()) and bool(full.any())
    # the returned mixes are the last forward's, at batch 3
    with torch.no_grad():
        again = console(tracks, *cap.params[-1], use_fx_bus=False)[1]
    assert G_same(out[0], again)


def test_one_song_against_a_profile_of_three_and_of_one():
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss, AudioFeatureProfile

    tracks, ref = songs((0, 1, 2))
    prof = AudioFeatureLoss(G.WEIGHTS, 44100).profile(ref)
    out, _, _ = fit(tracks[0], prof, 5, capture=False, batch=3)
    last = out[7]["loss"][-1].tolist()
    assert out[8] == [None] * 3 and len(set(last)) == 3, last
    one = AudioFeatureProfile(AudioFeatureLoss(G.WEIGHTS, 44100).profile(ref[:1]).data.cpu(), 44100).to(DEV)  # as a stored one comes back
    a, _, _ = fit(tracks[0], one, 3, capture=False, batch=2)
    b, _, _ = fit(tracks[0], ref[0], 3, capture=False, batch=2)  # a (2, M) tensor: profiled once, one reference for every item
    assert tuple(a[0].shape) == (2, 2, 32768) and a[8] == [None, None]
    assert G_same(a[1], b[1]) and torch.equal(a[7]["loss"], b[7]["loss"])
    assert not torch.equal(a[7]["loss"][:, 0], a[7]["loss"][:, 1])  # two start points


def test_no_host_wait_inside_the_loop():
    import test_online_gpu as G
    from mst import online
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole

    tracks, ref = songs((0, 1, 2))
    console, loss = AdvancedMixConsole(44100, validate="deferred"), AudioFeatureLoss(G.WEIGHTS, 44100)
    online.optimize_batch(tracks, ref, console, loss, n_iters=1)  # the constant tables of console and loss are built on their first call
    torch.manual_seed(0)
    r = online._Run(tracks, ref, console, loss, 0.001, LR, 5, (0.9, 0.999), 1e-8, None, None, {}, batched=True)  # the profile is taken here
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for n in range(5):
            r.iterate(n)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    out = r.finish()  # the one read
    console.check_parameters()
    history = out[7]["loss"]
    assert tuple(history.shape) == (5, 3) and bool((history[-1] < history[0]).all())  # and the loop did its work


class Poison:
    """callback: NaN into the track gradient of the chosen items at one iteration."""

    def __init__(self, items, at):
        self.items, self.at = items, at

    def __call__(self, n, view):
        if n == self.at:
            for b in self.items:
                view.grads[0][b, 1, 3] = float("nan")


def test_a_stopped_item_is_reported_and_the_others_finish():
    clean = three_songs()[0]
    tracks, ref = songs((0, 1, 2))
    out, _, _ = fit(tracks, ref, 5, callback=Poison((1,), 2))
    assert out[8] == [None, 2, None]
    for i in (1, 3, 5):
        assert bool(torch.isfinite(out[i]).all())
        for b in (0, 2):
            assert G_same(out[i][b], clean[i][b])
    assert torch.equal(out[7]["loss"][:, [0, 2]], clean[7]["loss"][:, [0, 2]])
    assert torch.equal(out[7]["loss"][:3, 1], clean[7]["loss"][:3, 1])  # item 1 up to and including the iteration that was refused
    with pytest.raises(FloatingPointError, match="every item"):
        fit(tracks, ref, 3, callback=Poison((0, 1, 2), 1))


def test_errors():
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss, MultiResolutionSTFTLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_batch

    tracks, ref = songs((0, 1))
    console = AdvancedMixConsole(44100)
    with pytest.raises(TypeError, match="per_item"):
        optimize_batch(tracks, ref, console, MultiResolutionSTFTLoss(), n_iters=1)
    loss = AudioFeatureLoss(G.WEIGHTS, 44100)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        optimize_batch(tracks.cpu(), ref, console, loss, n_iters=1)
    with pytest.raises(ValueError, match="n_iters"):
        optimize_batch(tracks, ref, console, loss, n_iters=0)
