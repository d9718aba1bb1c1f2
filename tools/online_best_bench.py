"""Keeping the best iterate: ``mst.online.optimize(keep_best=True)`` against ``optimize`` as it was before the best-iterate step existed.

    python tools/online_best_bench.py --baseline PARENT_TREE [--tracks 16] [--samples 524288] [--warmup 5] [--iters 50] [--rounds 3]
                                      [--passes 2] [--out FILE.json]

``PARENT_TREE`` is a built checkout of the parent commit (``git worktree add DIR HEAD~1`` and its ``__graft_entry__.build()``): the
baseline is that commit's ``optimize``, not this tree's with the flag off, which is measured as well.  Every measurement runs in a child
process of its own (one library per process; this process never opens the device); the three configurations alternate, ``passes`` times.

In a child: per-iteration time is a host clock from a synchronise in front of iteration ``warmup`` to a synchronise behind the last of
``iters`` more, of ONE run (the loop of ``optimize`` itself: ``_Run.iterate``), ``rounds`` runs; the console is
``validate="deferred"``, so nothing in the loop waits.  ``finish()`` - the read of the history and, with ``keep_best``, the init launch
and the console forward of the best logits - is timed on its own between two synchronises.  Launches are counted in separate passes
under torch's profiler, never in a timed one: device kernels and memory copies of whole ``optimize`` calls of 4 and of 7 iterations;
a third of the difference is one iteration, the rest of the shorter call is set-up and ``finish()``.  Needs the MI355X: there is no
CPU path.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [0.1, 0.001, 1.0, 1.0, 1.0]


def worker(a):
    root = os.path.abspath(a.root)
    sys.path[:0] = [root, os.path.join(root, "diff-mst_amd"), os.path.join(root, "diff-mst_amd", "standalone")]
    import torch

    from mst import online
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole

    assert os.path.abspath(online.__file__).startswith(root), online.__file__
    kw = dict(keep_best=True) if a.worker == "keep_best" else {}
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tracks = (0.1 * torch.randn(a.tracks, a.samples)).to(dev)
    loss_function = AudioFeatureLoss(WEIGHTS, 44100)
    with torch.no_grad():
        shapes = ((1, a.tracks, 27), (1, 25), (1, 26))
        ref_mix = AdvancedMixConsole(44100)(tracks[None], *(torch.rand(s, device=dev) * 0.5 + 0.25 for s in shapes),
                                            use_fx_bus=False)[1][0].clone()
    console = AdvancedMixConsole(44100, validate="deferred")

    def run(n_iters):
        torch.manual_seed(1)
        return online.optimize(tracks, ref_mix, console, loss_function, lr=1e-3, n_iters=n_iters, **kw)

    def one_round():
        """(ms per iteration of iterations [warmup, warmup + iters), ms of finish()) of one run; the loop is optimize()'s own."""
        torch.manual_seed(1)
        r = online._Run(tracks, ref_mix, console, loss_function, 0.001, 1e-3, a.warmup + a.iters, (0.9, 0.999), 1e-8, None, None, {}, **kw)
        for n in range(r.n_iters):
            if n == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            r.iterate(n)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = r.finish()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert all(v == v for v in out[7]["loss"]), "a loss was NaN"
        return (t1 - t0) * 1e3 / a.iters, (t2 - t1) * 1e3

    run(2)  # constant tables, allocator
    ms, fin = (list(column) for column in zip(*[one_round() for _ in range(a.rounds)]))
    try:  # whole runs of 1 + 3 and 1 + 6 iterations: their difference is three iterations without set-up and finish()
        from torch.profiler import ProfilerActivity, profile

        counts = []
        for n_iters in (4, 7):
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                run(n_iters)
                torch.cuda.synchronize()
            counts.append(sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")))
        if not counts[0]:
            raise RuntimeError("the profiler recorded no device activity")
        per_iter, outside = (counts[1] - counts[0]) / 3.0, counts[0] - 4 * (counts[1] - counts[0]) / 3.0
    except Exception as e:  # the profiler is not part of the measurement of time
        print(f"launches not measured: {e!r}", file=sys.stderr)
        per_iter = outside = None
    print("RESULT " + json.dumps(dict(ms=ms, finish_ms=fin, launches_per_iter=per_iter, launches_outside_loop=outside)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    ap.add_argument("--worker", default=None, choices=("plain", "keep_best"), help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    configs = [("optimize", HERE, "plain"), ("optimize(keep_best=True)", HERE, "keep_best")]
    if a.baseline:
        configs.insert(0, ("parent commit's optimize", os.path.abspath(a.baseline), "plain"))
    else:
        print("no --baseline: the parent commit's optimize is not measured")
    got = {name: dict(ms=[], finish_ms=[], launches_per_iter=None, launches_outside_loop=None) for name, _, _ in configs}
    for _ in range(a.passes):
        for name, root, mode in configs:  # alternating within a pass
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--root", root, "--tracks", str(a.tracks), "--samples",
                   str(a.samples), "--warmup", str(a.warmup), "--iters", str(a.iters), "--rounds", str(a.rounds)]
            out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
            res = json.loads(next(line for line in out.splitlines() if line.startswith("RESULT "))[7:])
            got[name]["ms"] += res["ms"]
            got[name]["finish_ms"] += res["finish_ms"]
            for key in ("launches_per_iter", "launches_outside_loop"):
                got[name][key] = res[key]
    result = dict(tracks=a.tracks, samples=a.samples, warmup=a.warmup, iters=a.iters, rounds=a.rounds, passes=a.passes, rows=[])
    for name, _, _ in configs:
        g = got[name]
        row = dict(loop=name, ms_per_iter=statistics.median(g["ms"]), ms_min=min(g["ms"]), ms_max=max(g["ms"]),
                   finish_ms=statistics.median(g["finish_ms"]), finish_min=min(g["finish_ms"]), finish_max=max(g["finish_ms"]),
                   launches_per_iter=g["launches_per_iter"], launches_outside_loop=g["launches_outside_loop"])
        result["rows"].append(row)
        shown = "not measured" if row["launches_per_iter"] is None else f"{row['launches_per_iter']:.1f}"
        print(f"{name:26s} T={a.tracks} N={a.samples}: {row['ms_per_iter']:.3f} ms / iteration (min {row['ms_min']:.3f}, max "
              f"{row['ms_max']:.3f} over {len(g['ms'])} runs of {a.iters}), finish() {row['finish_ms']:.3f} ms (min {row['finish_min']:.3f}, "
              f"max {row['finish_max']:.3f}), launches / iteration {shown}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
