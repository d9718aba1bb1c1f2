"""Per-song optimisation: ``mst.online.optimize`` against the same loop written as the reference's scripts/online.py writes it
(``torch.sigmoid``, ``torch.optim.Adam``, ``.item()`` per term), both on this package's console and ``AudioFeatureLoss``.

    python tools/online_bench.py [--tracks 16] [--samples 524288] [--warmup 5] [--iters 50] [--rounds 3] [--out FILE.json]

Per-iteration time is a host clock around ``iters`` iterations that end in a device synchronise (the script's loop stalls the host six
times per iteration, so the host clock is the one that counts), after ``warmup`` iterations of the same run; the two loops alternate
within a round and the median over the rounds is reported, with the spread.  Launches per iteration are counted in a separate pass under
torch's profiler (device kernels and memory copies of three iterations), never in a timed one.  Needs the MI355X: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-mst_amd"), os.path.join(ROOT, "diff-mst_amd", "standalone")]
import torch  # noqa: E402

from mst.loss import AudioFeatureLoss  # noqa: E402
from mst.modules import AdvancedMixConsole  # noqa: E402
from mst.online import optimize  # noqa: E402

WEIGHTS = [0.1, 0.001, 1.0, 1.0, 1.0]  # the script's, without the CLAP term


def script_loop(tracks, ref_mix, mix_console, loss_function, n_iters, lr, mark):
    """The loop of scripts/online.py:36-106 on this package's console and loss, line for line but for tqdm."""
    loss_history = {"loss": []}
    track_params = (0.001 * torch.randn(tracks.shape[0], 27)).type_as(tracks).requires_grad_(True)
    fx_bus_params = (0.001 * torch.randn(1, 25)).type_as(tracks).requires_grad_(True)
    master_bus_params = (0.001 * torch.randn(1, 26)).type_as(tracks).requires_grad_(True)
    optimizer = torch.optim.Adam([track_params, fx_bus_params, master_bus_params], lr=lr)
    tracks, ref_mix = tracks.unsqueeze(0), ref_mix.unsqueeze(0)
    for n in range(n_iters):
        mark(n)
        optimizer.zero_grad()
        result = mix_console(tracks, torch.sigmoid(track_params.unsqueeze(0)), torch.sigmoid(fx_bus_params),
                             torch.sigmoid(master_bus_params), use_fx_bus=False)
        loss = 0
        losses = loss_function(result[1], ref_mix)
        for loss_value in losses.values():
            loss += loss_value
        loss.backward()
        optimizer.step()
        loss_history["loss"].append(loss.item())
        for loss_name, loss_value in losses.items():
            loss_history.setdefault(loss_name, []).append(loss_value.item())
    return loss_history


def device_loop(tracks, ref_mix, mix_console, loss_function, n_iters, lr, mark):
    return optimize(tracks, ref_mix, mix_console, loss_function, lr=lr, n_iters=n_iters, callback=lambda n, view: mark(n))[7]


def timed(loop, args, warmup, iters):
    """ms per iteration of iterations [warmup, warmup + iters) of one run of ``loop``."""
    t0 = []

    def mark(n):
        if n == warmup:
            torch.cuda.synchronize()
            t0.append(time.perf_counter())

    history = loop(*args, warmup + iters, 1e-3, mark)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0[0]) * 1e3 / iters, history["loss"]


def launches(loop, args, iters=3):
    """Device kernels and memory copies per iteration, from a profiled pass of ``iters`` iterations after one untraced run."""
    from torch.profiler import ProfilerActivity, profile

    loop(*args, 2, 1e-3, lambda n: None)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        loop(*args, iters, 1e-3, lambda n: None)
        torch.cuda.synchronize()
    device = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    if not device:
        raise RuntimeError("the profiler recorded no device activity")
    return len(device) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("online_bench needs the MI355X")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tracks = (0.1 * torch.randn(a.tracks, a.samples)).to(dev)
    loss_function = AudioFeatureLoss(WEIGHTS, 44100)
    with torch.no_grad():
        ref_mix = AdvancedMixConsole(44100)(tracks[None], *(torch.rand(s, device=dev) * 0.5 + 0.25 for s in ((1, a.tracks, 27), (1, 25), (1, 26))),
                                            use_fx_bus=False)[1][0].clone()
    loops = {"script": script_loop, "optimize": device_loop}
    result = dict(tracks=a.tracks, samples=a.samples, warmup=a.warmup, iters=a.iters, rounds=a.rounds, rows=[])
    for validate in ("sync", "deferred"):
        console = AdvancedMixConsole(44100, validate=validate)
        args = (tracks, ref_mix, console, loss_function)
        ms = {name: [] for name in loops}
        for _ in range(a.rounds):
            for name, loop in loops.items():  # alternating within a round
                torch.manual_seed(1)
                t, history = timed(loop, args, a.warmup, a.iters)
                ms[name].append(t)
                assert all(v == v for v in history), "a loss was NaN"
        for name, loop in loops.items():
            try:
                count = launches(loop, args)
            except Exception as e:  # the profiler is not part of the measurement of time
                count = None
                print(f"launches per iteration of {name} not measured: {e!r}")
            row = dict(loop=name, validate=validate, ms_per_iter=statistics.median(ms[name]), ms_min=min(ms[name]), ms_max=max(ms[name]),
                       launches_per_iter=count)
            result["rows"].append(row)
            shown = "not measured" if count is None else f"{count:.1f}"
            print(f"{name:9s} validate={validate:9s} T={a.tracks} N={a.samples}: {row['ms_per_iter']:.3f} ms / iteration "
                  f"(min {row['ms_min']:.3f}, max {row['ms_max']:.3f} over {a.rounds} runs of {a.iters}), launches / iteration {shown}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
