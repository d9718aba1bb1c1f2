"""A batch of sectioned fits: ``mst.online.optimize_sections_batch`` at (B, S) = (1, 1), (2, 2), (4, 2), (2, 4) against the two loops
that a tree without it offers: B consecutive ``mst.online.optimize_sections`` calls at S, and ``mst.online.optimize_batch`` at batch
B * S (the same console and transform work, B * S independent parameter sets).  One song of T tracks, sections of N samples, one
stored ``AudioFeatureProfile``, ``validate="deferred"``.

    python tools/online_sections_batch_bench.py [--tracks 16] [--samples 524288] [--warmup 5] [--iters 30] [--rounds 3]
                                                [--shapes 1x1,2x2,4x2,2x4] [--root TREE] [--baseline-only] [--baseline FILE.json]
                                                [--md FILE.md] [--out FILE.json]

``--root TREE`` imports the package from another checkout (a build of the parent commit) and ``--baseline-only`` measures only the two
baselines, which every tree since DESIGN 23 has: the parent's figures are taken by this file in a process of their own and handed to
the run on this tree with ``--baseline``.  Without ``--baseline`` the baselines are measured on this tree.

Per-iteration time is tools/online_sections_bench.py's clock: a host clock from a synchronise in front of iteration ``warmup`` to a
synchronise behind the last iteration of ONE run of ``warmup + iters``, divided by ``iters``; "B consecutive calls" is the sum of B
such runs.  The loops alternate within a round and the median over the rounds is reported with the spread.  Launches per iteration
(device kernels and memory copies) are counted in a separate pass of three iterations under torch's profiler, never in a timed one.
No threshold is applied: the table is written whatever it shows.  Needs the MI355X: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _root():
    for i, arg in enumerate(sys.argv):
        if arg == "--root" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
        if arg.startswith("--root="):
            return os.path.abspath(arg.split("=", 1)[1])
    return HERE


ROOT = _root()
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-mst_amd"), os.path.join(ROOT, "diff-mst_amd", "standalone")]
import torch  # noqa: E402

from mst import online  # noqa: E402
from mst.loss import AudioFeatureLoss  # noqa: E402
from mst.modules import AdvancedMixConsole  # noqa: E402

WEIGHTS = [0.1, 0.001, 1.0, 1.0, 1.0]  # tools/online_bench.py's


def sections_batch_loop(items, profile, console, loss, n_iters, mark):
    """items (B, S, T, N)"""
    return online.optimize_sections_batch(items, profile, console, loss, lr=1e-3, n_iters=n_iters,
                                          callback=lambda n, view: mark(n))[7]["loss"]


def sections_loop(items, profile, console, loss, n_iters, mark):
    """ONE of the B consecutive calls: item 0's sections."""
    return torch.tensor(online.optimize_sections(items[0], profile, console, loss, lr=1e-3, n_iters=n_iters,
                                                 callback=lambda n, view: mark(n))[7]["loss"])


def batch_loop(items, profile, console, loss, n_iters, mark):
    """B * S independent single-section fits: the same rows through the console and the transforms."""
    rows = items.reshape((-1,) + tuple(items.shape[2:]))
    return online.optimize_batch(rows, profile, console, loss, lr=1e-3, n_iters=n_iters, callback=lambda n, view: mark(n))[7]["loss"]


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


def table(a):
    lines = [
        "# A batch of sectioned fits: `mst.online.optimize_sections_batch` against consecutive `optimize_sections` calls and `optimize_batch` (DESIGN §24)",
        "",
        f"`python tools/online_sections_batch_bench.py` on one MI355X.  One song of T = {a['tracks']} tracks cut into sections of N = "
        f"{a['samples']} samples; every item of a batch is S of them, fitted to one stored `AudioFeatureProfile`; `AudioFeatureLoss` "
        "weights `[0.1, 0.001, 1, 1, 1]`, `use_fx_bus=False`, lr 1e-3, `validate=\"deferred\"`.  \"optimize_sections_batch\" fits B "
        "parameter sets to S sections each in one call (one console forward at batch B S, the pooled loss with `items=B`, one step "
        "launch of B workgroups).  The baselines: B consecutive `optimize_sections` calls at S (the sum of B runs), and `optimize_batch` "
        f"at batch B S, which does the same console and transform work.  Baselines: {a['baseline_source']}.",
        "",
        f"Time: a host clock from a synchronise in front of iteration {a['warmup']} to a synchronise behind iteration "
        f"{a['warmup'] + a['iters'] - 1} of ONE run of {a['warmup'] + a['iters']}, divided by {a['iters']}; {a['rounds']} runs each, median "
        "(min, max).  Launches: device kernels and memory copies per iteration, counted in a separate pass of three iterations under "
        "torch's profiler, never in a timed pass (for the consecutive calls: of ONE call).  No threshold is applied to these figures.",
        "",
        "| B | S | optimize_sections_batch, ms / iteration | B consecutive optimize_sections, ms / iteration | optimize_batch at B S, ms / iteration | batch / consecutive | batch / optimize_batch | launches / iteration: optimize_sections_batch | one optimize_sections | optimize_batch |",
        "|---|---|---|---|---|---|---|---|---|---|",
    ]
    fmt = lambda r: "-" if r is None else f"{r['median']:.3f} ({r['min']:.3f}, {r['max']:.3f})"
    shown = lambda c: "-" if c is None else f"{c:.1f}"
    base = {(row["B"], row["S"]): row for row in a["baseline"]}
    for row in a["rows"]:
        b = base.get((row["B"], row["S"]), {})
        ratio = lambda key: "-" if not b.get(key) else f"{row['sections_batch']['median'] / b[key]['median']:.3f}"
        lines.append(f"| {row['B']} | {row['S']} | {fmt(row['sections_batch'])} | {fmt(b.get('consecutive'))} | {fmt(b.get('batch'))} | "
                     f"{ratio('consecutive')} | {ratio('batch')} | {shown(row['launches_sections_batch'])} | "
                     f"{shown(b.get('launches_sections'))} | {shown(b.get('launches_batch'))} |")
    lines += ["", "A ratio below 1: the batch of sectioned fits is cheaper per iteration than that baseline.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="1x1,2x2,4x2,2x4", help="BxS, comma separated")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is measured")
    ap.add_argument("--baseline-only", action="store_true", help="measure optimize_sections and optimize_batch only")
    ap.add_argument("--baseline", default=None, help="JSON of a --baseline-only run (another build) to set beside this tree's figures")
    ap.add_argument("--md", default=os.path.join(HERE, "profiles", "online_sections_batch.md"), help="where the table is written")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("online_sections_batch_bench needs the MI355X")
    dev = torch.device("cuda:0")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    rows_needed = max(B * S for B, S in shapes)
    torch.manual_seed(0)
    song = (0.1 * torch.randn(a.tracks, rows_needed * a.samples)).to(dev)
    loss = AudioFeatureLoss(WEIGHTS, 44100)
    with torch.no_grad():
        ref_mix = AdvancedMixConsole(44100)(song[None, :, :a.samples], *(torch.rand(s, device=dev) * 0.5 + 0.25
                                                                         for s in ((1, a.tracks, 27), (1, 25), (1, 26))),
                                            use_fx_bus=False)[1].clone()
    profile = loss.profile(ref_mix)
    console = AdvancedMixConsole(44100, validate="deferred")
    stat = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))
    result = dict(tracks=a.tracks, samples=a.samples, warmup=a.warmup, iters=a.iters, rounds=a.rounds, rows=[], baseline=[],
                  baseline_source="measured on this build, alternating with optimize_sections_batch within a round")
    given = None
    if a.baseline:
        with open(a.baseline) as f:
            given = json.load(f)
        result["baseline"] = given["baseline"]
        result["baseline_source"] = "a build of the parent commit, measured by this tool in a process of its own in the same session"
    for B, S in shapes:
        items = torch.stack([song[:, r * a.samples:(r + 1) * a.samples] for r in range(B * S)]).reshape(B, S, a.tracks, a.samples).contiguous()
        args = (items, profile, console, loss)
        mine, consecutive, batch = [], [], []
        for _ in range(a.rounds):  # alternating within a round
            if not a.baseline_only:
                torch.manual_seed(1)
                mine.append(timed(sections_batch_loop, args, a.warmup, a.iters))
            if given is None:
                torch.manual_seed(1)
                consecutive.append(sum(timed(sections_loop, (items[b:b + 1],) + args[1:], a.warmup, a.iters) for b in range(B)))
                torch.manual_seed(1)
                batch.append(timed(batch_loop, args, a.warmup, a.iters))
        if given is None:
            result["baseline"].append(dict(B=B, S=S, consecutive=stat(consecutive), batch=stat(batch),
                                           launches_sections=counted(sections_loop, args), launches_batch=counted(batch_loop, args)))
            print(f"B={B} S={S}: {B} consecutive optimize_sections {result['baseline'][-1]['consecutive']['median']:.3f}, optimize_batch "
                  f"{result['baseline'][-1]['batch']['median']:.3f} ms per iteration", flush=True)
        if not a.baseline_only:
            result["rows"].append(dict(B=B, S=S, sections_batch=stat(mine), launches_sections_batch=counted(sections_batch_loop, args)))
            print(f"B={B} S={S}: optimize_sections_batch {result['rows'][-1]['sections_batch']['median']:.3f} ms per iteration", flush=True)
        if a.out:  # after every shape: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)
    if not a.baseline_only:
        md = table(result)
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write(md)
        print(md)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
