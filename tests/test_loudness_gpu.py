"""The device loudness meter on the MI355X: production shapes against the float64 restatement of pyloudnorm's algorithm
(tests/loudness_ref.py; parity with the package itself is UNPINNED), the pyloudnorm-style ``LoudnessMeter``, ``run_diffmst`` with
``loudness_fn="device"``, and stream / graph behaviour.  Bounds and the gate-margin pre-check are those of
tests/test_loudness_hostsim.py."""
import os

import numpy as np
import pytest
import torch

import loudness_ref as R
from util import StubModel, rel

pytestmark = pytest.mark.gpu

FP32_ALLOWANCE_LU = 8.7e-5   # derived in tests/test_loudness_hostsim.py: a tenth of run_diffmst's 1e-4 mix tolerance, in LU
GATE_MARGIN_LU = 1e-3


def device_noise(rows, chs, n, seed, dev):
    """The level-step recipe of loudness_ref.level_step_noise, drawn on the device (512 x 131072 rows)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = 0.1 * torch.randn(rows, chs, n, generator=g, device=dev)
    x[..., int(0.2 * n):int(0.55 * n)] *= 10.0 ** (-30.0 / 20.0)
    x[..., int(0.55 * n):int(0.9 * n)] *= 1e-6
    x *= (10.0 ** (-0.7 * (torch.arange(rows, device=dev) % 16) / 20.0)).view(-1, 1, 1)
    return x


@pytest.mark.parametrize("rows,chs,n,rate,seed", [(16, 1, 262144, 44100, 101), (512, 1, 131072, 44100, 102), (8, 2, 262144, 48000, 103)])
def test_production_shapes_match_the_restatement(rows, chs, n, rate, seed, record):
    from mst.utils import integrated_loudness

    dev = torch.device("cuda:0")
    x = device_noise(rows, chs, n, seed, dev)
    lufs, blocks = integrated_loudness(x, rate, return_blocks=True)
    assert lufs.shape == (rows,) and lufs.is_cuda and blocks.shape == (rows, R.num_blocks(n, rate))
    again = integrated_loudness(x, rate)
    assert torch.equal(lufs, again)  # deterministic
    pick = list(range(0, rows, max(1, rows // 16)))[:16]  # the restatement runs on at most 16 rows
    xs = x[pick].cpu().numpy()
    lufs, blocks = lufs.double().cpu().numpy(), blocks.double().cpu().numpy()
    assert np.all(np.isfinite(lufs))
    err_l = err_b = 0.0
    for i, r in enumerate(pick):
        ref_l, ref_b = R.integrated_loudness(xs[i].T.astype(np.float64), rate, return_blocks=True)
        m_rel, m_abs = R.gate_margins(ref_b)
        assert m_rel > GATE_MARGIN_LU and m_abs > GATE_MARGIN_LU, f"row {r}: a block sits on a gate, change the seed"
        err_l = max(err_l, abs(lufs[r] - ref_l))
        err_b = max(err_b, float(np.max(np.abs(blocks[r] - ref_b)[ref_b > R.ABS_GATE])))
        a, _, f = R.gate_sets(blocks[r])
        ra, _, rf = R.gate_sets(ref_b)
        assert a == ra and f == rf
        assert 0 < len(rf) < len(ra) < len(ref_b)  # both gates remove blocks
    print(f"\n[{rows}x{chs}x{n} @ {rate}] |L - L_f64| = {err_l:.3e} LU, per block = {err_b:.3e} LU (bound {FP32_ALLOWANCE_LU:.1e})")
    record(lufs=err_l, block=err_b)
    assert err_l <= FP32_ALLOWANCE_LU and err_b <= FP32_ALLOWANCE_LU


def test_strided_views_and_leading_dimensions():
    from mst.utils import integrated_loudness, loudness_normalize

    dev = torch.device("cuda:0")
    long = device_noise(6, 2, 90001, 104, dev)
    crop = long[..., 3:3 + 70001]               # unaligned rows, n % 4 != 0
    a = integrated_loudness(crop)
    b = integrated_loudness(crop.contiguous())
    assert torch.equal(a, b)
    c = integrated_loudness(crop.contiguous().view(2, 3, 2, 70001))
    assert c.shape == (2, 3) and torch.equal(c.flatten(), a)
    one = integrated_loudness(crop[0])           # (channels, n) -> 0-dim
    assert one.shape == () and torch.equal(one, a[0])
    # normalisation: gains from the meter's own output, dropped rows are zeros
    x = crop.clone()
    x[1] = 0.0
    x[2] *= 1e-4
    y, lufs, keep = loudness_normalize(x, -23.0, floor_lufs=-80.0)
    assert y.shape == x.shape and keep.tolist() == [True, False, False, True, True, True]
    assert torch.isfinite(y).all() and not y[1].any() and not y[2].any()
    gain = (10.0 ** ((-23.0 - lufs.double()) / 20.0)).float().view(-1, 1, 1)
    k = keep.nonzero().flatten()
    assert torch.allclose(y[k], x[k] * gain[k], rtol=2.0 ** -22, atol=0.0)
    assert (integrated_loudness(y[k]) + 23.0).abs().max().item() < 1e-4
    with pytest.raises(NotImplementedError):
        integrated_loudness(crop.clone().requires_grad_())
    with torch.no_grad():
        integrated_loudness(crop.clone().requires_grad_())


def test_loudness_meter_is_a_drop_in_for_the_host_meter():
    from mst.utils import LoudnessMeter, integrated_loudness

    dev = torch.device("cuda:0")
    data = R.level_step_noise(1, 2, 100000, 105)[0].T.copy()  # numpy (n, 2), what pyloudnorm takes
    meter = LoudnessMeter(44100)
    got = meter.integrated_loudness(data)
    assert type(got) is float
    assert got == integrated_loudness(torch.from_numpy(data.T.copy()).to(dev)).item()
    assert abs(got - R.integrated_loudness(data, 44100)) <= FP32_ALLOWANCE_LU
    mono = meter.integrated_loudness(data[:, 0])                 # (n,)
    assert mono == meter.integrated_loudness(torch.from_numpy(data[:, :1]))  # host tensor (n, 1)
    with pytest.raises(ValueError, match="Audio must have length greater than the block size."):
        meter.integrated_loudness(data[:17639])


def test_run_diffmst_with_the_device_meter(golden_dir, record):
    """The fixture's track recipe; against the same driver with the float64 restatement injected as the host meter."""
    from mst.modules import AdvancedMixConsole
    from mst.utils import LoudnessMeter, run_diffmst

    dev = torch.device("cuda:0")
    g = np.load(os.path.join(golden_dir, "run_diffmst.npz"))
    T, n = (int(v) for v in g["shape"])
    torch.manual_seed(int(g["seed_tracks"]))
    tracks = (0.05 * torch.randn(1, T, n) * torch.tensor([1.0, 0.3, 2.0, 1e-6, 0.7]).view(1, T, 1)).half().float()
    ref = 0.2 * torch.randn(1, 2, int(g["ref_len"]))
    model = StubModel(seed=int(g["seed_model"])).to(dev)
    kw = dict(track_start_idx=int(g["track_start_idx"]), ref_start_idx=int(g["ref_start_idx"]))
    before = tracks.clone()
    host_meter = lambda a: R.integrated_loudness(a, 44100)
    want, wtpd, _, _ = run_diffmst(tracks, ref, model, AdvancedMixConsole(44100), loudness_fn=host_meter, **kw)
    got, tpd, _, mpd = run_diffmst(tracks, ref, model, AdvancedMixConsole(44100), loudness_fn="device", **kw)
    assert got.shape == (1, 2, n) and got.device == tracks.device and torch.equal(tracks, before)
    # both drop the 1e-6 track at the -80 LUFS floor
    assert tpd["compressor"]["ratio"].shape == (1, 4) and wtpd["compressor"]["ratio"].shape == (1, 4)
    assert torch.allclose(tpd["compressor"]["ratio"], wtpd["compressor"]["ratio"], rtol=1e-5)
    err = rel(got, want)
    print("\n[run_diffmst device meter vs float64 host meter] rel(mix) =", err)
    record(mix=err)
    assert err <= 1e-4
    # device tensors in -> device tensor out, same numbers
    again, *_ = run_diffmst(tracks.to(dev), ref.to(dev), model, AdvancedMixConsole(44100), loudness_fn="device", **kw)
    assert again.is_cuda and torch.equal(again.cpu(), got)
    # the pyloudnorm-style meter as loudness_fn: the same loudness values through the host loop.  The gains may differ in their last
    # fp32 place (10^x formed by the device's pow there, by Python here: 6e-8 relative); a tenth of the driver's 1e-4 bound covers
    # what the console's compressor makes of that
    via, *_ = run_diffmst(tracks, ref, model, AdvancedMixConsole(44100), loudness_fn=LoudnessMeter(44100).integrated_loudness, **kw)
    assert rel(via, got) <= 1e-5


def test_streams_and_graph_capture():
    from mst.utils import integrated_loudness

    dev = torch.device("cuda:0")
    x = device_noise(8, 1, 131072, 106, dev)
    eager, eager_b = integrated_loudness(x, return_blocks=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        s, s_b = integrated_loudness(x, return_blocks=True)
    side.synchronize()
    assert torch.equal(s, eager) and torch.equal(s_b, eager_b)
    # one linear chain of launches: capture and replay; a call that synchronised with the host could not be captured
    graph = torch.cuda.CUDAGraph()
    static_x = x.clone()
    with torch.cuda.graph(graph):
        out = integrated_loudness(static_x)
    static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static_x.mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert (out - (eager + 20.0 * np.log10(0.5))).abs().max().item() < 1e-4
