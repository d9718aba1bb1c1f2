"""Batched fits: ``mst.online.optimize_batch`` at B = 1, 2, 4, 8 against B consecutive ``mst.online.optimize`` calls (the loop a user
writes without it), one song of T tracks x N samples against one stored ``AudioFeatureProfile`` - the random-restart case.

    python tools/online_batch_bench.py [--tracks 16] [--samples 524288] [--warmup 5] [--iters 50] [--rounds 3] [--batches 1,2,4,8]
                                       [--md profiles/online_batch.md] [--out FILE.json]

One process.  Per-iteration time is a host clock from a synchronise in front of iteration ``warmup`` to a synchronise behind the last
iteration of ONE run of ``warmup + iters``, divided by ``iters`` (tools/online_bench.py's clock).  "B x optimize" runs B such
``optimize`` calls one after the other and adds their per-iteration times: what one iteration of all B fits costs when they are looped.
The two alternate within a round; the median over the rounds is reported with the spread.  Launches per iteration (device kernels and
memory copies) are counted in a separate pass of three iterations under torch's profiler, never in a timed one.  No threshold is
applied: the table is written whatever it shows.  Needs the MI355X: there is no CPU path.
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
from mst.online import optimize, optimize_batch  # noqa: E402

WEIGHTS = [0.1, 0.001, 1.0, 1.0, 1.0]  # tools/online_bench.py's


def batch_loop(B):
    def loop(tracks, profile, console, loss, n_iters, mark):
        return optimize_batch(tracks, profile, console, loss, lr=1e-3, n_iters=n_iters, batch=B, callback=lambda n, view: mark(n))[7]["loss"]

    return loop


def single_loop(tracks, profile, console, loss, n_iters, mark):
    return torch.tensor(optimize(tracks, profile, console, loss, lr=1e-3, n_iters=n_iters, callback=lambda n, view: mark(n))[7]["loss"])


def timed(loop, args, warmup, iters):
    """ms per iteration of iterations [warmup, warmup + iters) of one run of ``loop``."""
    t0 = []

    def mark(n):
        if n == warmup:
            torch.cuda.synchronize()
            t0.append(time.perf_counter())

    history = loop(*args, warmup + iters, mark)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0[0]) * 1e3 / iters
    assert bool(torch.isfinite(history).all()), "a loss was not finite"
    return ms


def launches(loop, args, iters=3):
    """Device kernels and memory copies per iteration, from a profiled pass of ``iters`` iterations after one untraced run."""
    from torch.profiler import ProfilerActivity, profile

    loop(*args, 2, lambda n: None)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        loop(*args, iters, lambda n: None)
        torch.cuda.synchronize()
    device = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    if not device:
        raise RuntimeError("the profiler recorded no device activity")
    return len(device) / iters


def counted(loop, args):
    try:
        return launches(loop, args)
    except Exception as e:  # the profiler is not part of the measurement of time
        print(f"launches per iteration not measured: {e!r}")
        return None


def table(result):
    a = result
    lines = [
        "# Batched fits: `mst.online.optimize_batch` against consecutive `optimize` calls (DESIGN §21)",
        "",
        f"`python tools/online_batch_bench.py` on one MI355X, one process.  One song of T = {a['tracks']} tracks, N = {a['samples']} samples "
        "fitted B times from B start points (random restarts) to one stored `AudioFeatureProfile`; `AudioFeatureLoss` weights "
        "`[0.1, 0.001, 1, 1, 1]`, `use_fx_bus=False`, lr 1e-3.  \"B x optimize\" is B `mst.online.optimize` calls one after the other - the "
        "loop this change replaces, unchanged since the parent commit - with their per-iteration times added; \"optimize_batch\" is one "
        "call at batch B.",
        "",
        f"Time: a host clock from a synchronise in front of iteration {a['warmup']} to a synchronise behind iteration "
        f"{a['warmup'] + a['iters'] - 1} of ONE run of {a['warmup'] + a['iters']}, divided by {a['iters']}; the two alternate, {a['rounds']} "
        "runs each, median (min, max).  Launches: device kernels and memory copies per iteration, counted in a separate pass of three "
        "iterations under torch's profiler, never in a timed pass.  No threshold is applied to these figures.",
        "",
        "| console | B | B x optimize, ms / iteration | optimize_batch, ms / iteration | ratio | ms / iteration / fit | launches / iteration: B x optimize | optimize_batch |",
        "|---|---|---|---|---|---|---|---|",
    ]
    fmt = lambda r: f"{r['median']:.3f} ({r['min']:.3f}, {r['max']:.3f})"
    shown = lambda c: "not measured" if c is None else f"{c:.1f}"
    for row in a["rows"]:
        s, b = row["serial"], row["batch"]
        lines.append(f"| `validate=\"{row['validate']}\"` | {row['B']} | {fmt(s)} | {fmt(b)} | {s['median'] / b['median']:.2f} x | "
                     f"{b['median'] / row['B']:.3f} | {shown(None if row['launches_single'] is None else row['B'] * row['launches_single'])} | "
                     f"{shown(row['launches_batch'])} |")
    lines += ["", "ratio = (B x optimize) / optimize_batch: above 1, the batch is cheaper than the loop; below 1, it is dearer.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "online_batch.md"), help="where the table is written")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("online_batch_bench needs the MI355X")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tracks = (0.1 * torch.randn(a.tracks, a.samples)).to(dev)
    loss = AudioFeatureLoss(WEIGHTS, 44100)
    with torch.no_grad():
        ref_mix = AdvancedMixConsole(44100)(tracks[None], *(torch.rand(s, device=dev) * 0.5 + 0.25 for s in ((1, a.tracks, 27), (1, 25), (1, 26))),
                                            use_fx_bus=False)[1].clone()
    profile = loss.profile(ref_mix)
    result = dict(tracks=a.tracks, samples=a.samples, warmup=a.warmup, iters=a.iters, rounds=a.rounds, rows=[])
    for validate in ("sync", "deferred"):
        console = AdvancedMixConsole(44100, validate=validate)
        args = (tracks, profile, console, loss)
        single_count = counted(single_loop, args)
        for B in [int(v) for v in a.batches.split(",")]:
            serial, batch = [], []
            for _ in range(a.rounds):  # alternating within a round
                torch.manual_seed(1)
                serial.append(sum(timed(single_loop, args, a.warmup, a.iters) for _ in range(B)))
                torch.manual_seed(1)
                batch.append(timed(batch_loop(B), args, a.warmup, a.iters))
            stat = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))
            row = dict(validate=validate, B=B, serial=stat(serial), batch=stat(batch), launches_single=single_count,
                       launches_batch=counted(batch_loop(B), args))
            result["rows"].append(row)
            print(f"validate={validate:9s} B={B}: {B} x optimize {row['serial']['median']:.3f} ms, optimize_batch {row['batch']['median']:.3f} ms "
                  f"per iteration ({row['serial']['median'] / row['batch']['median']:.2f} x)", flush=True)
    md = table(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as f:
        f.write(md)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(md)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
