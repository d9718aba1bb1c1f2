"""One parameter set fitted to several sections on the MI355X: the step cases of tests/test_online_sections_hostsim.py
(tests/online_sections_ref.py) through the C ABI of the product library, then ``mst.online.optimize_sections`` end to end - one section
bit for bit ``optimize``, two sections replayed through the host reference step, ``pooled`` as the loop's loss, no host wait inside the
loop, ``render_blocks``, ``keep_best`` - and descent.  T = 3, n = 32768, the signals and weights of tests/test_online_gpu.py."""
import functools

import pytest
import torch

import online_ref as O
import online_sections_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ITERS, LR = 20, 1e-3


@pytest.fixture()
def drv():
    from mst import _hip

    d = O.Driver(_hip.lib(), DEV)
    yield d
    from online_batch_ref import scrub

    scrub(d)


# ---- the kernels through the C ABI: the simulator's cases --------------------------------------------------------------------------
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


# ---- optimize_sections() end to end ------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and torch.equal(O.bits(a), O.bits(b))


@functools.lru_cache(maxsize=None)
def sectioned_song(seed):
    """(whole tracks (T, 2 N), its two sections (2, T, N), the pooled profile of its reference mix's two sections) on the device."""
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss
    from mst.online import take_sections

    tracks, ref = G.song(seed, G.T, 2 * G.N)
    sections = take_sections(tracks, (0, G.N), G.N)
    assert tuple(sections.shape) == (2, G.T, G.N) and sections.is_contiguous() and same_bits(sections[1], tracks[:, G.N:])
    target = AudioFeatureLoss(G.WEIGHTS, 44100).profile(torch.stack((ref[:, :G.N], ref[:, G.N:])), pool=True)
    assert target.batch_size == 1 and target.n_samples == 2 * G.N
    return tracks, sections, target


def counting_loss(weights, sample_rate):
    """An AudioFeatureLoss that counts what the loop calls, in ``calls``."""
    from mst.loss import AudioFeatureLoss

    class Counting(AudioFeatureLoss):
        def forward(self, *a, **k):
            self.calls["forward"] += 1
            return super().forward(*a, **k)

        def per_item(self, *a, **k):
            self.calls["per_item"] += 1
            return super().per_item(*a, **k)

        def pooled(self, *a, **k):
            self.calls["pooled"] += 1
            return super().pooled(*a, **k)

        def profile(self, *a, **k):
            self.calls["profile"] += 1
            return super().profile(*a, **k)

    loss = Counting(weights, sample_rate)
    loss.calls = dict(forward=0, per_item=0, pooled=0, profile=0)
    return loss


def fit(seed, n_iters=ITERS, capture=True, **kw):
    import test_online_gpu as G
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_sections

    _, sections, target = sectioned_song(seed)
    console, cap, loss = AdvancedMixConsole(44100), G.Capture() if capture else None, counting_loss(G.WEIGHTS, 44100)
    torch.manual_seed(seed)
    out = optimize_sections(sections, target, console, loss, n_iters=n_iters, lr=LR, callback=cap, **kw)
    return out, cap, console, loss


@functools.lru_cache(maxsize=None)
def captured(seed):
    """One captured run per seed, shared by the cases below and never modified."""
    return fit(seed)


def test_one_section_is_optimize_bit_for_bit():
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize, optimize_sections

    tracks, ref = G.song(0)
    loss = AudioFeatureLoss(G.WEIGHTS, 44100)
    stored = loss.profile(ref[None])
    torch.manual_seed(0)
    single = optimize(tracks, stored, AdvancedMixConsole(44100), loss, n_iters=5, lr=LR)
    torch.manual_seed(0)
    got = optimize_sections(tracks[None], stored, AdvancedMixConsole(44100), loss, n_iters=5, lr=LR)
    assert len(got) == len(single) == 8 and tuple(got[0].shape) == (1, 2, G.N)
    assert same_bits(got[0][0], single[0])
    for i in (1, 3, 5):
        assert same_bits(got[i], single[i])
    assert got[7] == single[7]


def test_two_sections_replay_through_the_host_step(record):
    import test_online_gpu as G

    out, cap, _, loss = captured(0)
    assert loss.calls == dict(forward=0, per_item=0, pooled=ITERS, profile=0)  # the stored profile: nothing to analyse
    assert [g is None for g in cap.grads[0]] == [False, True, False]  # use_fx_bus=False: the fx parameters have no gradient
    assert [tuple(g.shape) for g in (cap.grads[0][0], cap.grads[0][2])] == [(2, G.T, 27), (2, 26)]
    assert [tuple(t.shape) for t in (out[0], out[1], out[3], out[5])] == [(2, 2, G.N), (1, G.T, 27), (1, 25), (1, 26)]
    for params in cap.params:  # the rows of every leaf are equal
        for p in params:
            assert same_bits(p[0], p[1])
    theta0 = [t.cpu().reshape(-1) for t in cap.logits[0]]
    stream = [None if cap.grads[0][s] is None else torch.stack([P.host_sum(g[s].cpu().reshape(2, -1)) for g in cap.grads]) for s in range(3)]
    t64 = O.adam_f64(theta0, stream, LR)
    e_torch = O.e_stat(O.adam_torch(theta0, stream, LR), t64, theta0)
    got = [out[1], out[3], out[5]]
    e_kernel, floor = O.e_stat(got, t64, theta0), O.floor_term(t64, theta0)
    print(f"\n[replay two sections] e(kernel) = {e_kernel:.3e}, e(torch fp32) = {e_torch:.3e}, floor {floor:.3e}")
    record(kernel=e_kernel, torch_fp32=e_torch, floor=floor)
    assert e_kernel <= O.SLACK * e_torch + floor
    assert same_bits(got[1].cpu().reshape(-1), theta0[1])
    # the history is the captured terms and their left-to-right fp32 sum
    history = out[7]
    keys = list(cap.losses[0])
    assert list(history) == ["loss"] + keys and len(keys) == 5
    for k, losses in enumerate(cap.losses):
        total = torch.zeros((), device=DEV)
        for name in keys:
            assert tuple(losses[name].shape) == (1,)
            total = total + losses[name][0]
            assert history[name][k] == float(losses[name])
        assert history["loss"][k] == float(total)


def test_a_tensor_reference_is_profiled_once():
    import test_online_gpu as G
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_sections

    _, sections, _ = sectioned_song(0)
    ref = G.song(0, G.T, 2 * G.N)[1]
    loss = counting_loss(G.WEIGHTS, 44100)
    torch.manual_seed(0)
    out = optimize_sections(sections, ref, AdvancedMixConsole(44100), loss, n_iters=3, lr=LR)
    assert loss.calls == dict(forward=0, per_item=0, pooled=3, profile=1) and len(out[7]["loss"]) == 3


def test_no_host_wait_inside_the_loop():
    import test_online_gpu as G
    from mst import online
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole

    _, sections, target = sectioned_song(0)
    console, loss = AdvancedMixConsole(44100, validate="deferred"), AudioFeatureLoss(G.WEIGHTS, 44100)
    online.optimize_sections(sections, target, console, loss, n_iters=1)  # the constant tables of console and loss are built on their first call
    torch.manual_seed(0)
    r = online._Run(sections, target, console, loss, 0.001, LR, ITERS, (0.9, 0.999), 1e-8, None, None, {}, sectioned=True)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for n in range(ITERS):
            r.iterate(n)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    out = r.finish()  # the one read
    console.check_parameters()
    history = out[7]["loss"]
    assert len(history) == ITERS and history[-1] < history[0]  # and the loop did its work
    assert same_bits(out[1], captured(0)[0][1])  # the same fit as the captured one


def test_the_result_feeds_render_blocks():
    import test_online_gpu as G
    from mst.online import render_blocks

    out, _, console, _ = captured(0)
    tracks, _, _ = sectioned_song(0)
    full = render_blocks(tracks, out[1], out[3], out[5], console, block_size=G.N)
    assert tuple(full.shape) == (2, 2 * G.N) and bool(torch.isfinite(full).all()) and bool(full[:, G.N:].any())


def test_keep_best_returns_the_console_output_at_the_returned_logits():
    from mst import online

    out, _, console, _ = fit(0, n_iters=8, capture=False, keep_best=True, patience=3)
    _, sections, _ = sectioned_song(0)
    assert len(out) == 9 and isinstance(out[8], online.FitReport) and tuple(out[0].shape) == tuple(sections.shape[:1]) + (2, sections.shape[2])
    logits = (out[1], out[3], out[5])
    params = tuple(torch.full((2,) + tuple(t.shape[1:]), float("nan"), device=DEV) for t in logits)
    online._init(logits, params, None, 2)
    with torch.no_grad():
        again = console(sections, *params, use_fx_bus=False)[1]
    assert same_bits(out[0], again)
    assert out[8].best_loss == min(out[7]["loss"][:out[8].iterations_run]) and out[7]["loss"][out[8].best_iteration] == out[8].best_loss


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_descent(seed, record):
    """Two sections against the pooled profile of their own reference mix, 20 iterations at lr 1e-3.  The project's 0.8 bound
    (tests/test_online_gpu.py): the measured ratios, 0.296 / 0.166 / 0.234 for seeds 0 / 1 / 2, are as wide of it as those
    of the single-section fits of DESIGN 19 (0.305 / 0.154 / 0.237)."""
    history = captured(seed)[0][7]["loss"]
    print(f"\n[optimize_sections seed {seed}] loss {history[0]:.4e} -> {history[-1]:.4e} (ratio {history[-1] / history[0]:.3f})")
    record(first=history[0], last=history[-1])
    assert len(history) == ITERS
    assert history[-1] < 0.8 * history[0]


def test_errors():
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss, MultiResolutionSTFTLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_sections

    _, sections, target = sectioned_song(0)
    console, loss = AdvancedMixConsole(44100), AudioFeatureLoss(G.WEIGHTS, 44100)
    with pytest.raises(TypeError, match="pooled"):
        optimize_sections(sections, target, console, MultiResolutionSTFTLoss(), n_iters=1)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        optimize_sections(sections.cpu(), target, console, loss, n_iters=1)
    with pytest.raises(ValueError, match="batch size"):
        loss.pooled(sections[:, :2], loss.profile(sections[:, :2]))
