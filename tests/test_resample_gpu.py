"""The device resampler on the MI355X through ``mst.utils.resample``: the cases of tests/test_resample_hostsim.py (float64
restatement of torchaudio's algorithm, tests/resample_ref.py - parity with the package itself is UNPINNED; closed form; adjoint;
determinism), one production shape, streams and graph replay, and ``run_diffmst`` on 48 kHz tracks."""
import os

import numpy as np
import pytest
import torch

import resample_ref as R
from resample_ref import RATIOS, RESTATEMENT_VS_CLOSED_FORM, SINE_RATIOS, case_lengths, check_forward, noise, sine_case
from util import StubModel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def frames_per_tile(orig, new):
    from mst.utils import _resample_tables

    return int(_resample_tables(torch.device(DEV), orig, new)[:64].cpu().view(torch.int32)[4])  # include/diffmst_hip.h


def guarded(x, orig, new):
    """resample() allocates its own output; what it returns must be complete (no NaN from an unwritten sample)."""
    from mst.utils import resample

    y = resample(x, orig, new)
    assert y.is_cuda and y.dtype == x.dtype and y.shape == x.shape[:-1] + (R.out_samples(x.shape[-1], orig, new),)
    assert torch.isfinite(y).all()
    return y


# ---- 1. + 2. values and lengths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", RATIOS)
def test_forward_matches_the_float64_restatement(orig, new, record):
    F = frames_per_tile(orig, new)
    assert F % 4 == 0 and F > 0
    fn = lambda v: guarded(v.to(DEV), orig, new)
    worst = 0.0
    for n in case_lengths(orig, new, F):
        worst = max(worst, check_forward(fn, orig, new, noise((1, n), 1000 + n), f"{orig}->{new} 1x{n}"))
    o, _ = R.reduced(orig, new)
    for n in (o + 1, 5003):
        x = noise((3, n), 2000 + n)
        worst = max(worst, check_forward(fn, orig, new, x, f"{orig}->{new} 3x{n}"))

        def strided(v):
            wide = noise((v.shape[0], v.shape[1] + 3), 999).to(DEV)
            wide[:, 1:-2] = v.to(DEV)
            view = wide[:, 1:-2]  # odd 4-byte alignment, row stride > length; read in place
            assert view.stride(0) == v.shape[1] + 3 and not view.is_contiguous()
            return guarded(view, orig, new)

        worst = max(worst, check_forward(strided, orig, new, x, f"{orig}->{new} 3x{n} strided"))
    worst = max(worst, check_forward(fn, orig, new, noise((2, 3, 5003), 3000), f"{orig}->{new} 2x3x5003"))
    record(err=worst, bound=R.forward_bound(orig, new))


def test_one_song_section():
    """8 x 524288 at 48000 -> 44100: against the float64 restatement, and the guard region behind a caller-owned output."""
    from mst import _hip
    from mst.utils import _resample_tables, resample

    orig, new, rows, n = 48000, 44100, 8, 524288
    x = noise((rows, n), 8000)
    check_forward(lambda v: guarded(v.to(DEV), orig, new), orig, new, x, f"{orig}->{new} {rows}x{n}")
    # the C ABI on a NaN-filled buffer with a guard region: every output written, nothing behind n_out
    lib, dev = _hip.lib(), torch.device(DEV)
    xd = x.to(dev)
    n_out = lib.mst_resample_out_samples(n, orig, new)
    assert n_out == R.out_samples(n, orig, new)
    buf = torch.full((rows * n_out + 4096,), float("nan"), device=dev)
    with _hip.launch_on(dev) as st:
        lib.mst_resample_forward(xd, rows, n, n, orig, new, _resample_tables(dev, orig, new), buf, st)
    assert torch.isnan(buf[rows * n_out:]).all()
    assert torch.equal(buf[: rows * n_out].view(rows, n_out), resample(xd, orig, new))


# ---- 3. closed form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", SINE_RATIOS)
def test_sine_matches_the_closed_form(orig, new, record):
    x, want, mid = sine_case(orig, new)
    ref = float((R.resample(x, orig, new, torch.float64) - want)[mid].abs().max())
    got = guarded(x.float().to(DEV), orig, new).double().cpu()
    err = float((got - want)[mid].abs().max())
    print(f"\n[997 Hz {orig}->{new}] restatement vs closed form {ref:.3e}, kernel {err:.3e}")
    record(restatement=ref, kernel=err)
    assert ref <= RESTATEMENT_VS_CLOSED_FORM
    assert err <= RESTATEMENT_VS_CLOSED_FORM + R.forward_bound(orig, new)


# ---- 4. adjoint ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", RATIOS)
def test_adjoint(orig, new, record):
    from mst.utils import resample

    o, _ = R.reduced(orig, new)
    for n in (o + 1, 5003):
        x = noise((3, n), 4000 + n)
        g = noise((3, R.out_samples(n, orig, new)), 5000 + n)
        want = R.adjoint(g, n, orig, new)
        xd = x.to(DEV).requires_grad_()
        y = resample(xd, orig, new)
        (gx,) = torch.autograd.grad(y, xd, g.to(DEV))
        assert gx.shape == x.shape and torch.isfinite(gx).all()
        gx, y = gx.cpu(), y.detach().cpu()
        bound_adj = R.adjoint_bound(orig, new, float(g.abs().max()))
        err = float((gx.double() - want).abs().max())
        print(f"\n[{orig}->{new} adjoint 3x{n}] |gx - gx_f64| = {err:.3e} (bound {bound_adj:.3e})")
        assert err <= bound_adj
        lhs, rhs = float((y.double() * g.double()).sum()), float((x.double() * gx.double()).sum())
        slack = R.forward_bound(orig, new, float(x.abs().max())) * float(g.abs().sum()) + bound_adj * float(x.abs().sum())
        print(f"[{orig}->{new} dot 3x{n}] <Ax, g> - <x, A^T g> = {lhs - rhs:.3e} (bound {slack:.3e})")
        assert abs(lhs - rhs) <= slack
    record(err=err, bound=R.adjoint_bound(orig, new))


# ---- 5. determinism, batching, streams, graph ---------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", [(48000, 44100), (44100, 48000), (44100, 8000)])
def test_bit_identical_calls_and_rows(orig, new):
    from mst.utils import resample

    x = noise((3, 5003), 6000).to(DEV)
    a, b = resample(x, orig, new), resample(x, orig, new)
    assert torch.equal(a, b)
    g = noise(tuple(a.shape), 6001).to(DEV)
    xa = x.clone().requires_grad_()
    (ga,) = torch.autograd.grad(resample(xa, orig, new), xa, g)
    xb = x.clone().requires_grad_()
    (gb,) = torch.autograd.grad(resample(xb, orig, new), xb, g)
    assert torch.equal(ga, gb)
    for r in range(3):
        xr = x[r:r + 1].clone().requires_grad_()
        yr = resample(xr, orig, new)
        assert torch.equal(yr[0], a[r])
        assert torch.equal(torch.autograd.grad(yr, xr, g[r:r + 1])[0][0], ga[r])


def test_streams_and_graph_capture():
    from mst.utils import resample

    dev = torch.device(DEV)
    x = noise((8, 131072), 6100).to(dev)
    eager = resample(x, 48000, 44100)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        s = resample(x, 48000, 44100)
    side.synchronize()
    assert torch.equal(s, eager)
    # one launch, no host synchronisation: capture and replay
    graph = torch.cuda.CUDAGraph()
    static_x = x.clone()
    with torch.cuda.graph(graph):
        out = resample(static_x, 48000, 44100)
    static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static_x.mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager * 0.5)  # a power of two scales every product and sum exactly


# ---- 6. edges -----------------------------------------------------------------------------------------------------------------
def test_edges():
    from mst.utils import Resample, resample

    x = noise((2, 1000), 6200).to(DEV)
    assert resample(x, 44100, 44100) is x and resample(x, 48000.0, 48000) is x and Resample(44100, 44100)(x) is x
    with pytest.raises(ValueError, match="44101"):
        resample(x, 44101, 44100)
    with pytest.raises(ValueError):
        resample(x, 44100.5, 44100)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        resample(x.cpu(), 48000, 44100)
    y = resample(x, 48000, 44100)
    assert torch.equal(Resample(48000, 44100)(x), y) and torch.equal(resample(x, 48000.0, 44100.0), y)
    assert torch.equal(resample(x, 96000, 88200), y)  # the same reduced ratio, the same table
    # other float dtypes: converted, computed in fp32, cast back
    for dt in (torch.float64, torch.bfloat16, torch.float16):
        yd = resample(x.to(dt), 48000, 44100)
        assert yd.dtype == dt and torch.equal(yd, resample(x.to(dt).float(), 48000, 44100).to(dt))
    xg = x.double().requires_grad_()
    resample(xg, 48000, 44100).sum().backward()
    assert xg.grad.dtype == torch.float64 and xg.grad.shape == xg.shape
    one = resample(x[0], 48000, 44100)  # (time,)
    assert one.shape == (y.shape[1],) and torch.equal(one, y[0])


# ---- 7. run_diffmst -----------------------------------------------------------------------------------------------------------
def test_run_diffmst_on_48k_tracks(golden_dir):
    """The model and track recipe of test_loudness_gpu.py::test_run_diffmst_with_the_device_meter, the tracks taken as 48 kHz
    material: converted inside the driver, and converted by the caller."""
    from mst.modules import AdvancedMixConsole
    from mst.utils import resample, run_diffmst

    dev = torch.device(DEV)
    g = np.load(os.path.join(golden_dir, "run_diffmst.npz"))
    T, n = (int(v) for v in g["shape"])
    torch.manual_seed(int(g["seed_tracks"]))
    tracks = (0.05 * torch.randn(1, T, n) * torch.tensor([1.0, 0.3, 2.0, 1e-6, 0.7]).view(1, T, 1)).half().float()
    ref = 0.2 * torch.randn(1, 2, int(g["ref_len"]))
    model = StubModel(seed=int(g["seed_model"])).to(dev)
    kw = dict(track_start_idx=int(g["track_start_idx"]), ref_start_idx=int(g["ref_start_idx"]), loudness_fn="device")
    before = tracks.clone()
    got, *_ = run_diffmst(tracks, ref, model, AdvancedMixConsole(44100), track_sample_rate=48000, **kw)
    converted = resample(tracks.to(dev), 48000, 44100)
    want, *_ = run_diffmst(converted, ref, model, AdvancedMixConsole(44100), **kw)
    assert got.shape == (1, 2, R.out_samples(n, 48000, 44100)) and got.device == tracks.device and torch.equal(tracks, before)
    assert torch.isfinite(got).all() and got.abs().max() > 0
    assert torch.equal(got, want.cpu())
    # the reference mix at another rate as well
    ref48 = 0.2 * torch.randn(1, 2, 300000)
    a, *_ = run_diffmst(tracks, ref48, model, AdvancedMixConsole(44100), track_sample_rate=48000, ref_sample_rate=48000, **kw)
    b, *_ = run_diffmst(converted, resample(ref48.to(dev), 48000, 44100), model, AdvancedMixConsole(44100), **kw)
    assert torch.equal(a, b.cpu())
