"""The per-item MR-STFT loss and the batched fits on it, in the pattern of tools/online_batch_bench.py.

    python tools/online_mrstft_batch_bench.py --baseline-only --package-root PARENT_CHECKOUT --out base.json
    python tools/online_mrstft_batch_bench.py --baseline base.json [--md profiles/online_mrstft_batch.md] [--out FILE.json]
                                              [--tracks 16] [--samples 524288] [--warmup 3] [--iters 15] [--rounds 3] [--batches 1,2,4,8]

Two measurements, both at T tracks x N samples, the reference's three resolutions, ``validate="deferred"``:

* the loss alone: ``per_item`` forward + backward at ``(B, 2, N)`` against the scalar ``forward`` + backward on the same rows.  The
  per-item path runs the scalar path's transform launches; it swaps the reduction's last body and adds one coefficient-scaling launch.
* the fits: ``optimize_batch`` with this loss at batch B against B consecutive ``optimize`` calls with their per-iteration times added.

The baselines - the scalar loss and the consecutive ``optimize`` calls, neither of which this feature touches - are taken on a build of
the PARENT commit: a first run with ``--baseline-only --package-root`` imports that checkout's package (its own library) and writes
them as JSON, a second run in the same session measures this checkout and takes them in with ``--baseline``; without ``--baseline``
the same baselines are measured on this checkout and labelled so.  One process per run.  Clocks: tools/online_batch_bench.py's (a
host clock between synchronises; the median over the rounds with the spread).  The time of one small launch is measured in the same
run as the increment of a back-to-back loop of one-element kernels.  Launches per iteration come from a separate profiled pass.  No
threshold is applied.  Needs the MI355X.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R3 = dict(fft_sizes=[512, 2048, 8192], hop_sizes=[256, 1024, 4096], win_lengths=[512, 2048, 8192])


def stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def clock(fn, reps):
    """ms per call of ``reps`` back-to-back calls between two synchronises, after one untimed call"""
    import torch

    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def loss_step(call, x, y, cotangent):
    def step():
        x.grad = None
        call(x, y).backward(cotangent)

    return step


def timed_fit(loop, warmup, iters):
    """ms per iteration of iterations [warmup, warmup + iters) of one run of ``loop(n_iters, mark)``"""
    import torch

    t0 = []

    def mark(n):
        if n == warmup:
            torch.cuda.synchronize()
            t0.append(time.perf_counter())

    history = loop(warmup + iters, mark)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0[0]) * 1e3 / iters
    assert bool(torch.isfinite(history).all()), "a loss was not finite"
    return ms


def launches(loop, iters=3):
    """device kernels and memory copies per iteration, from a profiled pass after one untraced run; None if the profiler fails"""
    import torch
    from torch.profiler import ProfilerActivity, profile

    try:
        loop(2, lambda n: None)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            loop(iters, lambda n: None)
            torch.cuda.synchronize()
        device = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        return len(device) / iters if device else None
    except Exception as e:  # the profiler is not part of the measurement of time
        print(f"launches per iteration not measured: {e!r}")
        return None


def fmt(r):
    return f"{r['median']:.3f} ({r['min']:.3f}, {r['max']:.3f})"


def table(a):
    shown = lambda c: "not measured" if c is None else f"{c:.1f}"
    base = a["baseline_build"]
    lines = [
        "# The per-item MR-STFT loss and batched fits on it (DESIGN §26)",
        "",
        f"`python tools/online_mrstft_batch_bench.py` on one MI355X.  T = {a['tracks']} tracks, N = {a['samples']} samples, the reference's "
        "resolutions (512 / 2048 / 8192, hop = n_fft / 2), `validate=\"deferred\"`, `use_fx_bus=False`, lr 1e-3.  Baselines (the scalar loss, "
        f"consecutive `optimize` calls): {base}, one process each, same session.  Times: a host clock between two synchronises; median "
        f"(min, max) over {a['rounds']} rounds.  One small launch (the increment of a back-to-back loop of one-element kernels, this "
        f"session): {a['small_launch_us']:.1f} us.  No threshold is applied to these figures.",
        "",
        "## The loss alone: `per_item` forward + backward at `(B, 2, N)` against the scalar loss on the same rows",
        "",
        "| B | scalar loss (baseline), ms | run-to-run spread of the baseline, ms | per_item, ms | difference, ms | difference - spread, us | in small launches |",
        "|---|---|---|---|---|---|---|",
    ]
    for row in a["loss_rows"]:
        s, p = row["scalar"], row["per_item"]
        spread, diff = s["max"] - s["min"], p["median"] - s["median"]
        lines.append(f"| {row['B']} | {fmt(s)} | {spread:.3f} | {fmt(p)} | {diff:+.3f} | {(diff - spread) * 1e3:+.1f} | "
                     f"{(diff - spread) * 1e3 / a['small_launch_us']:+.1f} |")
    lines += [
        "",
        "## The fits: `optimize_batch` at batch B against B consecutive `optimize` calls, the same loss",
        "",
        "| B | B x optimize (baseline), ms / iteration | optimize_batch, ms / iteration | ratio | ms / iteration / fit | launches / iteration: B x optimize | optimize_batch |",
        "|---|---|---|---|---|---|---|",
    ]
    for row in a["fit_rows"]:
        s, b = row["serial"], row["batch"]
        lines.append(f"| {row['B']} | {fmt(s)} | {fmt(b)} | {s['median'] / b['median']:.2f} x | {b['median'] / row['B']:.3f} | "
                     f"{shown(None if row['launches_single'] is None else row['B'] * row['launches_single'])} | {shown(row['launches_batch'])} |")
    lines += ["", "ratio = (B x optimize) / optimize_batch: above 1, the batch is cheaper than the loop; below 1, it is dearer.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loss-reps", type=int, default=30)
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--package-root", default=HERE, help="the checkout whose package (and library) is imported")
    ap.add_argument("--baseline-only", action="store_true", help="measure the baselines alone (for a parent checkout) and write --out")
    ap.add_argument("--baseline", default=None, help="JSON of a --baseline-only run on the parent build")
    ap.add_argument("--md", default=os.path.join(HERE, "profiles", "online_mrstft_batch.md"), help="where the table is written")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    root = os.path.abspath(a.package_root)
    sys.path[:0] = [root, os.path.join(root, "diff-mst_amd"), os.path.join(root, "diff-mst_amd", "standalone")]
    import torch

    from mst.loss import MultiResolutionSTFTLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize

    if not torch.cuda.is_available():
        raise SystemExit("online_mrstft_batch_bench needs the MI355X")
    dev = torch.device("cuda:0")
    batches = [int(v) for v in a.batches.split(",")]
    torch.manual_seed(0)
    tracks = (0.1 * torch.randn(a.tracks, a.samples)).to(dev)
    loss = MultiResolutionSTFTLoss(**R3)
    console = AdvancedMixConsole(44100, validate="deferred")
    with torch.no_grad():
        ref_mix = AdvancedMixConsole(44100)(tracks[None], *(torch.rand(s, device=dev) * 0.5 + 0.25 for s in ((1, a.tracks, 27), (1, 25), (1, 26))),
                                            use_fx_bus=False)[1][0].clone()
    tick = torch.zeros(1, device=dev)
    small = [(clock(lambda: [tick.add_(1.0) for _ in range(200)], 5) - clock(lambda: [tick.add_(1.0) for _ in range(100)], 5)) * 10.0
             for _ in range(a.rounds)]
    result = dict(tracks=a.tracks, samples=a.samples, warmup=a.warmup, iters=a.iters, rounds=a.rounds, loss_reps=a.loss_reps,
                  small_launch_us=statistics.median(small), package_root=root, loss_rows=[], fit_rows=[])

    def single_loop(n_iters, mark):
        return torch.tensor(optimize(tracks, ref_mix, console, loss, lr=1e-3, n_iters=n_iters, callback=lambda n, view: mark(n))[7]["loss"])

    single_count = launches(single_loop)
    for B in batches:
        torch.manual_seed(2)
        x = (0.3 * torch.randn(B, 2, a.samples, device=dev)).requires_grad_(True)
        y = 0.5 * x.detach() + 0.2 * torch.randn(B, 2, a.samples, device=dev)
        scalar = [clock(loss_step(loss, x, y, torch.ones((), device=dev)), a.loss_reps) for _ in range(a.rounds)]
        serial = []
        for _ in range(a.rounds):
            torch.manual_seed(1)
            serial.append(sum(timed_fit(single_loop, a.warmup, a.iters) for _ in range(B)))
        result["loss_rows"].append(dict(B=B, scalar=stat(scalar)))
        result["fit_rows"].append(dict(B=B, serial=stat(serial), launches_single=single_count))
        print(f"baselines B={B}: scalar loss {stat(scalar)['median']:.3f} ms, {B} x optimize {stat(serial)['median']:.3f} ms / iteration", flush=True)
    if a.baseline_only:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
        return
    result["baseline_build"] = "measured on THIS build (no --baseline given)"
    if a.baseline:
        with open(a.baseline) as f:
            base = json.load(f)
        for key in ("tracks", "samples", "warmup", "iters", "rounds", "loss_reps"):
            assert base[key] == result[key], f"the baseline was measured with another {key}"
        result["own_baselines"] = dict(loss_rows=result["loss_rows"], fit_rows=result["fit_rows"])  # the same figures on this build, kept
        result["loss_rows"], result["fit_rows"] = base["loss_rows"], base["fit_rows"]
        result["baseline_build"] = "a build of the parent commit"
    from mst.online import optimize_batch

    for B, lrow, frow in zip(batches, result["loss_rows"], result["fit_rows"]):
        assert lrow["B"] == frow["B"] == B
        torch.manual_seed(2)
        x = (0.3 * torch.randn(B, 2, a.samples, device=dev)).requires_grad_(True)
        y = 0.5 * x.detach() + 0.2 * torch.randn(B, 2, a.samples, device=dev)
        lrow["per_item"] = stat([clock(loss_step(loss.per_item, x, y, torch.ones(B, device=dev)), a.loss_reps) for _ in range(a.rounds)])

        def batch_loop(n_iters, mark, B=B):
            return optimize_batch(tracks, ref_mix, console, loss, lr=1e-3, n_iters=n_iters, batch=B, callback=lambda n, view: mark(n))[7]["loss"]

        batch = []
        for _ in range(a.rounds):
            torch.manual_seed(1)
            batch.append(timed_fit(batch_loop, a.warmup, a.iters))
        frow["batch"], frow["launches_batch"] = stat(batch), launches(batch_loop)
        print(f"B={B}: per_item {lrow['per_item']['median']:.3f} ms (scalar {lrow['scalar']['median']:.3f}), optimize_batch "
              f"{frow['batch']['median']:.3f} ms / iteration ({B} x optimize {frow['serial']['median']:.3f})", flush=True)
    md = table(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as f:
        f.write(md)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(md)


if __name__ == "__main__":
    main()
