"""Linked stereo pairs in a fit: ``mst.online.optimize`` with eight stereo pairs (``stereo_id``) against the same call without links,
and the call without links against a build of the parent commit.  One song of T tracks and N samples, one stored
``AudioFeatureProfile``, ``validate="deferred"``.

    python tools/online_links_bench.py [--tracks 16] [--samples 524288] [--warmup 5] [--iters 30] [--rounds 5] [--root TREE]
                                       [--unlinked-only] [--parent FILE.json ...] [--md FILE.md] [--out FILE.json]

``--root TREE`` imports the package from another checkout (a build of the parent commit) and ``--unlinked-only`` measures only the call
without links, which every tree since DESIGN 18 has: the parent's figures are taken by this file in processes of their own and handed to
the run on this tree with ``--parent`` (several files: several runs of the parent, whose medians show its run-to-run spread).

Per-iteration time is tools/online_sections_batch_bench.py's clock: a host clock from a synchronise in front of iteration ``warmup`` to
a synchronise behind the last iteration of ONE run of ``warmup + iters``, divided by ``iters``.  The two loops alternate within a round
and the median over the rounds is reported with the spread.  Launches per iteration (device kernels and memory copies) are counted in
a separate pass of three iterations under torch's profiler, never in a timed one.  No threshold is applied: the table is written
whatever it shows.  Needs the MI355X: there is no CPU path.
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


def loop(tracks, profile, console, loss, extra, n_iters, mark):
    return torch.tensor(online.optimize(tracks, profile, console, loss, lr=1e-3, n_iters=n_iters, callback=lambda n, view: mark(n),
                                        **extra)[7]["loss"])


def timed(args, warmup, iters):
    """ms per iteration of iterations [warmup, warmup + iters) of one run."""
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


def launches(args, iters=3):
    """Device kernels and memory copies per iteration, from a profiled pass of ``iters`` iterations after one untraced run."""
    from torch.profiler import ProfilerActivity, profile

    try:
        loop(*args, 2, lambda n: None)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            loop(*args, iters, lambda n: None)
            torch.cuda.synchronize()
        device = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        if not device:
            raise RuntimeError("the profiler recorded no device activity")
        return len(device) / iters
    except Exception as e:  # the profiler is not part of the measurement of time
        print(f"launches per iteration not measured: {e!r}")
        return None


def table(a):
    fmt = lambda r: "-" if r is None else f"{r['median']:.3f} ({r['min']:.3f}, {r['max']:.3f})"
    shown = lambda c: "-" if c is None else f"{c:.1f}"
    lines = [
        "# Linked stereo pairs: `mst.online.optimize(..., stereo_id=...)` against the fit without links and against the parent commit (DESIGN §25)",
        "",
        f"`python tools/online_links_bench.py` on one MI355X.  One song of T = {a['tracks']} tracks and N = {a['samples']} samples fitted "
        "to one stored `AudioFeatureProfile`; `AudioFeatureLoss` weights `[0.1, 0.001, 1, 1, 1]`, `use_fx_bus=False`, lr 1e-3, "
        f"`validate=\"deferred\"`.  \"linked\": `stereo_id = [1, 0] * {a['tracks'] // 2}`, {a['tracks'] // 2} stereo pairs with a mirrored pan "
        "(`mst_logit_adam_step_linked`).  \"no links\": the same call without the keyword (`mst_logit_adam_step`, the call a tree "
        "without the feature makes).  \"parent\": the call without links on a build of the parent commit, measured by this tool in "
        "processes of their own in the same session.",
        "",
        f"Time: a host clock from a synchronise in front of iteration {a['warmup']} to a synchronise behind iteration "
        f"{a['warmup'] + a['iters'] - 1} of ONE run of {a['warmup'] + a['iters']}, divided by {a['iters']}; {a['rounds']} runs each, alternating, "
        "median (min, max).  Launches: device kernels and memory copies per iteration, counted in a separate pass of three iterations "
        "under torch's profiler, never in a timed pass.  No threshold is applied to these figures.",
        "",
        "| configuration | ms / iteration | launches / iteration |",
        "|---|---|---|",
    ]
    for k, parent in enumerate(a["parent"]):
        lines.append(f"| parent commit, no links (process {k + 1}) | {fmt(parent['unlinked'])} | {shown(parent['launches_unlinked'])} |")
    lines.append(f"| this tree, no links | {fmt(a['unlinked'])} | {shown(a['launches_unlinked'])} |")
    if a.get("linked"):
        lines.append(f"| this tree, {a['tracks'] // 2} stereo pairs linked | {fmt(a['linked'])} | {shown(a['launches_linked'])} |")
    lines.append("")
    if a["parent"]:
        medians = [p["unlinked"]["median"] for p in a["parent"]]
        lo, hi = min(p["unlinked"]["min"] for p in a["parent"]), max(p["unlinked"]["max"] for p in a["parent"])
        lines.append(f"The parent's medians: {', '.join(f'{m:.3f}' for m in medians)} ms (between processes "
                     f"{max(medians) - min(medians):.3f} ms apart); all of its runs lie in [{lo:.3f}, {hi:.3f}] ms.  This tree without links: "
                     f"{a['unlinked']['median']:.3f} ms.")
    if a.get("linked"):
        lines.append(f"Linked minus no links on this tree: {a['linked']['median'] - a['unlinked']['median']:+.3f} ms per iteration.")
    lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--root", default=HERE, help="the checkout whose package is measured")
    ap.add_argument("--unlinked-only", action="store_true", help="measure the call without links only (a tree without the feature)")
    ap.add_argument("--parent", action="append", default=[], help="JSON of an --unlinked-only run of another build; may be repeated")
    ap.add_argument("--md", default=os.path.join(HERE, "profiles", "online_links.md"), help="where the table is written")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("online_links_bench needs the MI355X")
    if a.tracks % 2:
        raise SystemExit("--tracks must be even: the song is cut into stereo pairs")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    song = (0.1 * torch.randn(a.tracks, a.samples)).to(dev)
    loss = AudioFeatureLoss(WEIGHTS, 44100)
    with torch.no_grad():
        ref_mix = AdvancedMixConsole(44100)(song[None], *(torch.rand(s, device=dev) * 0.5 + 0.25 for s in ((1, a.tracks, 27), (1, 25), (1, 26))),
                                            use_fx_bus=False)[1].clone()
    profile = loss.profile(ref_mix)
    console = AdvancedMixConsole(44100, validate="deferred")
    stat = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))
    unlinked_args = (song, profile, console, loss, {})
    linked_args = (song, profile, console, loss, dict(stereo_id=[1, 0] * (a.tracks // 2)))
    unlinked, linked = [], []
    for _ in range(a.rounds):  # alternating within a round
        torch.manual_seed(1)
        unlinked.append(timed(unlinked_args, a.warmup, a.iters))
        if not a.unlinked_only:
            torch.manual_seed(1)
            linked.append(timed(linked_args, a.warmup, a.iters))
    result = dict(tracks=a.tracks, samples=a.samples, warmup=a.warmup, iters=a.iters, rounds=a.rounds, root=os.path.basename(ROOT),
                  unlinked=stat(unlinked), launches_unlinked=launches(unlinked_args), parent=[])
    if not a.unlinked_only:
        result.update(linked=stat(linked), launches_linked=launches(linked_args))
    for path in a.parent:
        with open(path) as f:
            result["parent"].append(json.load(f))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    if not a.unlinked_only:
        md = table(result)
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write(md)
        print(md)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
