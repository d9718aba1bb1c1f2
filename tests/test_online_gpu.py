"""Per-song optimisation on the MI355X: the cases of tests/test_online_hostsim.py on the device (through the C ABI of the product
library, tests/online_ref.py), then ``mst.online.optimize`` end to end - descent, a replay of its captured gradients through the float64
recurrence and torch's Adam, exact consistencies, no host wait inside the loop, a loss that returns a tensor - ``render_blocks`` and
the errors.  Parity with the reference's scripts/online.py is restated and UNPINNED (the script cannot be imported)."""
import functools

import pytest
import torch

import online_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, N, ITERS, LR = 3, 32768, 20, 1e-3
WEIGHTS = [0.1, 0.001, 1.0, 1.0, 1.0]
SEEDS = (0, 1, 2)


@pytest.fixture()
def drv():
    from mst import _hip

    return R.Driver(_hip.lib(), DEV)


# ---- the kernels through the C ABI: the simulator's cases -----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.STREAMS))
def test_step_matches_adam_behind_sigmoid(drv, name, record):
    R.check_parity(drv, name, record)


@pytest.mark.parametrize("count", R.TAIL_COUNTS)
def test_lane_tails_and_the_loop(drv, count):
    R.check_parity(drv, str(count))


def test_sigmoid(drv, record):
    R.check_sigmoid(drv, record)


def test_null_gradient_and_zero_gradient_keep_their_bits(drv):
    R.check_unchanged_bits(drv)


@pytest.mark.parametrize("where", ["gradient", "loss"])
def test_nonfinite_input_stops_the_step_and_is_reported(drv, where):
    R.check_nonfinite(drv, where)


@pytest.mark.parametrize("n_terms", [1, 5])
def test_history_rows(drv, n_terms):
    R.check_history(drv, n_terms)


# ---- optimize() end to end ------------------------------------------------------------------------------------------------------
def coloured_tracks(n_tracks, n, seed):
    """White, pink, brown ... noise (spectral slope f^(-k/2) for track k), each at -20 dBFS rms."""
    g = torch.Generator().manual_seed(1000 + seed)
    spec = torch.fft.rfft(torch.randn(n_tracks, n, generator=g, dtype=torch.float64))
    f = torch.arange(spec.shape[1], dtype=torch.float64).clamp_min(1.0)
    x = torch.fft.irfft(spec * f ** (-0.5 * torch.arange(n_tracks, dtype=torch.float64)[:, None]), n=n)
    return (0.1 * x / x.pow(2).mean(dim=1, keepdim=True).sqrt()).float()


@functools.lru_cache(maxsize=None)
def song(seed, n_tracks=T, n=N):
    """(tracks (T, n), ref_mix (2, n)) on the device: the reference mix is this console's output for parameters from [0.25, 0.75]."""
    from mst.modules import AdvancedMixConsole

    g = torch.Generator().manual_seed(2000 + seed)
    tracks = coloured_tracks(n_tracks, n, seed).to(DEV)
    tp, fp, mp = (0.25 + 0.5 * torch.rand(shape, generator=g) for shape in ((1, n_tracks, 27), (1, 25), (1, 26)))
    with torch.no_grad():
        ref = AdvancedMixConsole(44100)(tracks[None], tp.to(DEV), fp.to(DEV), mp.to(DEV), use_fx_bus=False)[1][0]
    return tracks, ref.clone()


class Capture:
    """callback of optimize(): clones of the live tensors of every iteration."""

    def __init__(self):
        self.params, self.grads, self.losses, self.logits = [], [], [], []

    def __call__(self, n, view):
        assert n == len(self.params)
        self.params.append([p.detach().clone() for p in view.params])
        self.grads.append([None if g is None else g.clone() for g in view.grads])
        losses = view.losses
        self.losses.append({k: v.detach().clone() for k, v in losses.items()} if isinstance(losses, dict) else losses.detach().clone())
        self.logits.append([t.clone() for t in view.logits])


def run(seed, capture=True):
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize

    tracks, ref = song(seed)
    console, cap = AdvancedMixConsole(44100), Capture() if capture else None
    torch.manual_seed(seed)
    out = optimize(tracks, ref, console, AudioFeatureLoss(WEIGHTS, 44100), n_iters=ITERS, lr=LR, callback=cap)
    return out, cap, console


@functools.lru_cache(maxsize=None)
def captured(seed):
    """One captured run per seed, shared by the cases below and never modified."""
    return run(seed)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(R.bits(a), R.bits(b))


@pytest.mark.parametrize("seed", SEEDS)
def test_descent(seed, record):
    history = captured(seed)[0][7]["loss"]
    print(f"\n[optimize seed {seed}] loss {history[0]:.4e} -> {history[-1]:.4e} (ratio {history[-1] / history[0]:.3f})")
    record(first=history[0], last=history[-1])
    assert len(history) == ITERS
    assert history[-1] < 0.8 * history[0]


@pytest.mark.parametrize("seed", SEEDS)
def test_replay_of_the_captured_gradients(seed, record):
    out, cap, _ = captured(seed)
    assert [g is None for g in cap.grads[0]] == [False, True, False]  # use_fx_bus=False: the fx parameters have no gradient
    theta0 = [t.cpu().reshape(-1) for t in cap.logits[0]]
    stream = [None if cap.grads[0][s] is None else torch.stack([g[s].cpu().reshape(-1) for g in cap.grads]) for s in range(3)]
    t64 = R.adam_f64(theta0, stream, LR)
    e_torch = R.e_stat(R.adam_torch(theta0, stream, LR), t64, theta0)
    got = [out[1], out[3], out[5]]
    e_kernel, floor = R.e_stat(got, t64, theta0), R.floor_term(t64, theta0)
    print(f"\n[replay seed {seed}] e(kernel) = {e_kernel:.3e}, e(torch fp32) = {e_torch:.3e}, floor {floor:.3e}")
    record(kernel=e_kernel, torch_fp32=e_torch, floor=floor)
    assert e_kernel <= R.SLACK * e_torch + floor
    assert same_bits(got[1].cpu().reshape(-1), theta0[1])  # no gradient: the fx logits are the start point's
    bound = R.sigmoid_bound()
    for params, logits in zip(cap.params, cap.logits):
        for p, th in zip(params, logits):
            assert R.ulps_from_f64(p.reshape(-1), torch.sigmoid(th.double().cpu().reshape(-1))) <= bound


def test_exact_consistencies():
    seed = 0
    out, cap, console = captured(seed)
    tracks, _ = song(seed)
    # the returned mix is the last forward's: before the last update
    with torch.no_grad():
        again = console(tracks[None], *cap.params[-1], use_fx_bus=False)[1][0]
    assert same_bits(out[0], again) and out[0].is_cuda
    # the history is the captured terms and their left-to-right fp32 sum
    history = out[7]
    keys = list(cap.losses[0])
    assert list(history) == ["loss"] + keys and len(keys) == 5
    for k, losses in enumerate(cap.losses):
        total = torch.zeros((), device=DEV)
        for name in keys:
            total = total + losses[name]
            assert history[name][k] == float(losses[name])
        assert history["loss"][k] == float(total)
    # the start point is the script's three draws
    torch.manual_seed(seed)
    draws = [0.001 * torch.randn(T, 27), 0.001 * torch.randn(1, 25), 0.001 * torch.randn(1, 26)]
    for th, d in zip(cap.logits[0], draws):
        assert same_bits(th.reshape(d.shape), d)
    assert [tuple(t.shape) for t in (out[1], out[3], out[5])] == [(1, T, 27), (1, 25), (1, 26)]
    # the dictionaries are the last forward's
    last = console._denormalized_dicts(*cap.params[-1])
    assert same_bits(out[2]["input_fader"]["gain_db"], last[0]["input_fader"]["gain_db"])
    assert same_bits(out[6]["output_fader"]["gain_db"], last[2]["output_fader"]["gain_db"])
    # a second run from the same seed
    out2, _, _ = run(seed, capture=False)
    assert same_bits(out2[0], out[0]) and out2[7] == history
    for i in (1, 3, 5):
        assert same_bits(out2[i], out[i])


def test_no_host_wait_inside_the_loop():
    from mst import online
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole

    tracks, ref = song(0)
    console, loss = AdvancedMixConsole(44100, validate="deferred"), AudioFeatureLoss(WEIGHTS, 44100)
    online.optimize(tracks, ref, console, loss, n_iters=1)  # the constant tables of console and loss are built on their first call
    torch.manual_seed(0)
    r = online._Run(tracks, ref, console, loss, 0.001, LR, ITERS, (0.9, 0.999), 1e-8, None, None, {})
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
    assert len(history) == ITERS and history[-1] < 0.8 * history[0]  # and the loop did its work


def test_a_loss_that_returns_a_tensor():
    from mst.loss import MultiResolutionSTFTLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize

    tracks, ref = song(0, T, 16384)
    console, cap = AdvancedMixConsole(44100), Capture()
    torch.manual_seed(0)
    out = optimize(tracks, ref, console, MultiResolutionSTFTLoss(), n_iters=3, callback=cap)
    assert list(out[7]) == ["loss"] and len(out[7]["loss"]) == 3
    assert out[7]["loss"] == [float(v) for v in cap.losses]
    with torch.no_grad():
        again = console(tracks[None], *cap.params[-1], use_fx_bus=False)[1][0]
    assert same_bits(out[0], again)


def test_render_blocks():
    from mst import online
    from mst.modules import AdvancedMixConsole
    from mst.online import render_blocks

    block, n = 8192, 2 * 8192 + 100
    tracks = coloured_tracks(2, n, 7).to(DEV)
    g = torch.Generator().manual_seed(7)
    logits = [torch.randn(shape, generator=g).to(DEV) for shape in ((1, 2, 27), (1, 25), (1, 26))]
    console = AdvancedMixConsole(44100)
    full = render_blocks(tracks, *logits, console, block_size=block)
    assert full.is_cuda and tuple(full.shape) == (2, n) and not bool(full[:, 2 * block:].any())
    params = [torch.full_like(t, float("nan")) for t in logits]
    online._init(logits, params)  # the kernel's sigmoid, as in optimize()
    for p, th in zip(params, logits):
        assert R.ulps_from_f64(p.reshape(-1), torch.sigmoid(th.double().cpu().reshape(-1))) <= R.sigmoid_bound()
    with torch.no_grad():
        for b in range(2):
            alone = console(tracks[:, b * block:(b + 1) * block].contiguous()[None], *params, use_fx_bus=False)[1][0]
            assert same_bits(full[:, b * block:(b + 1) * block], alone)


def test_errors():
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize, render_blocks

    tracks, ref = song(0)
    console, loss = AdvancedMixConsole(44100), AudioFeatureLoss(WEIGHTS, 44100)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        optimize(tracks.cpu(), ref, console, loss, n_iters=1)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        optimize(tracks, ref.cpu(), console, loss, n_iters=1)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        render_blocks(tracks.cpu(), torch.zeros(1, T, 27), torch.zeros(1, 25), torch.zeros(1, 26), console)
    with pytest.raises(ValueError):
        optimize(tracks[None], ref, console, loss, n_iters=1)
    bad = ref.clone()
    bad[0, 1234] = float("nan")
    with pytest.raises(FloatingPointError, match="iteration 0"):
        optimize(tracks, bad, console, loss, n_iters=2)
