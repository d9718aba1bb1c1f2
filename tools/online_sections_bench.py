"""Sectioned fits: ``mst.online.optimize_sections`` at S = 1, 2, 4, 8 sections against the two loops that do the same console and
transform work: ``mst.online.optimize`` (S = 1) and ``mst.online.optimize_batch`` at B = S.  One song of T tracks, sections of N
samples, one stored ``AudioFeatureProfile``, ``validate="deferred"``.

    python tools/online_sections_bench.py [--tracks 16] [--samples 524288] [--warmup 5] [--iters 30] [--rounds 3] [--sections 1,2,4,8]
                                          [--root TREE] [--baseline-only] [--baseline FILE.json] [--md FILE.md] [--out FILE.json]

``--root TREE`` imports the package from another checkout (a build of the parent commit) and ``--baseline-only`` measures only the two
baselines, which every tree since DESIGN 21 has: the parent's figures are taken by this file in a process of their own and handed to
the run on this tree with ``--baseline``.  Without ``--baseline`` the baselines are measured on this tree.

Per-iteration time is a host clock from a synchronise in front of iteration ``warmup`` to a synchronise behind the last iteration of
ONE run of ``warmup + iters``, divided by ``iters`` (tools/online_batch_bench.py's clock); the loops alternate within a round and the
median over the rounds is reported with the spread.  Launches per iteration (device kernels and memory copies) are counted in a
separate pass of three iterations under torch's profiler, never in a timed one.  No threshold is applied: the table is written
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


def sections_loop(sections, profile, console, loss, n_iters, mark):
    return torch.tensor(online.optimize_sections(sections, profile, console, loss, lr=1e-3, n_iters=n_iters,
                                                 callback=lambda n, view: mark(n))[7]["loss"])


def batch_loop(sections, profile, console, loss, n_iters, mark):
    return online.optimize_batch(sections, profile, console, loss, lr=1e-3, n_iters=n_iters, callback=lambda n, view: mark(n))[7]["loss"]


def single_loop(sections, profile, console, loss, n_iters, mark):
    return torch.tensor(online.optimize(sections[0], profile, console, loss, lr=1e-3, n_iters=n_iters,
                                        callback=lambda n, view: mark(n))[7]["loss"])


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
        "# Sectioned fits: `mst.online.optimize_sections` against `optimize` and `optimize_batch` (DESIGN §23)",
        "",
        f"`python tools/online_sections_bench.py` on one MI355X.  One song of T = {a['tracks']} tracks cut into S sections of N = "
        f"{a['samples']} samples, fitted to one stored `AudioFeatureProfile`; `AudioFeatureLoss` weights `[0.1, 0.001, 1, 1, 1]`, "
        "`use_fx_bus=False`, lr 1e-3, `validate=\"deferred\"`.  \"optimize_sections\" fits ONE parameter set to the S sections (pooled "
        "loss, one step workgroup that sums the S gradient rows).  The baselines do the same console and transform work: \"optimize\" "
        f"on one section (S = 1) and \"optimize_batch\" at B = S (S independent parameter sets).  Baselines: {a['baseline_source']}.",
        "",
        f"Time: a host clock from a synchronise in front of iteration {a['warmup']} to a synchronise behind iteration "
        f"{a['warmup'] + a['iters'] - 1} of ONE run of {a['warmup'] + a['iters']}, divided by {a['iters']}; {a['rounds']} runs each, median "
        "(min, max).  Launches: device kernels and memory copies per iteration, counted in a separate pass of three iterations under "
        "torch's profiler, never in a timed pass.  No threshold is applied to these figures.",
        "",
        "| S | optimize_sections, ms / iteration | optimize (S = 1), ms / iteration | optimize_batch at B = S, ms / iteration | sections / batch | launches / iteration: optimize_sections | optimize | optimize_batch |",
        "|---|---|---|---|---|---|---|---|",
    ]
    fmt = lambda r: "-" if r is None else f"{r['median']:.3f} ({r['min']:.3f}, {r['max']:.3f})"
    shown = lambda c: "-" if c is None else f"{c:.1f}"
    base = {row["S"]: row for row in a["baseline"]}
    for row in a["rows"]:
        b = base.get(row["S"], {})
        ratio = "-" if not b.get("batch") else f"{row['sections']['median'] / b['batch']['median']:.3f}"
        lines.append(f"| {row['S']} | {fmt(row['sections'])} | {fmt(b.get('single'))} | {fmt(b.get('batch'))} | {ratio} | "
                     f"{shown(row['launches_sections'])} | {shown(b.get('launches_single'))} | {shown(b.get('launches_batch'))} |")
    lines += ["", "sections / batch below 1: the sectioned fit is cheaper per iteration than the batch of S independent fits.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=16)
    ap.add_argument("--samples", type=int, default=524288)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sections", default="1,2,4,8")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is measured")
    ap.add_argument("--baseline-only", action="store_true", help="measure optimize and optimize_batch only")
    ap.add_argument("--baseline", default=None, help="JSON of a --baseline-only run (another build) to set beside this tree's figures")
    ap.add_argument("--md", default=os.path.join(HERE, "profiles", "online_sections.md"), help="where the table is written")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("online_sections_bench needs the MI355X")
    dev = torch.device("cuda:0")
    counts = [int(v) for v in a.sections.split(",")]
    torch.manual_seed(0)
    song = (0.1 * torch.randn(a.tracks, max(counts) * a.samples)).to(dev)
    loss = AudioFeatureLoss(WEIGHTS, 44100)
    with torch.no_grad():
        ref_mix = AdvancedMixConsole(44100)(song[None, :, :a.samples], *(torch.rand(s, device=dev) * 0.5 + 0.25
                                                                         for s in ((1, a.tracks, 27), (1, 25), (1, 26))),
                                            use_fx_bus=False)[1].clone()
    profile = loss.profile(ref_mix)
    console = AdvancedMixConsole(44100, validate="deferred")
    stat = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))
    result = dict(tracks=a.tracks, samples=a.samples, warmup=a.warmup, iters=a.iters, rounds=a.rounds, rows=[], baseline=[],
                  baseline_source="measured on this build, alternating with optimize_sections within a round")
    given = None
    if a.baseline:
        with open(a.baseline) as f:
            given = json.load(f)
        result["baseline"] = given["baseline"]
        result["baseline_source"] = "a build of the parent commit, measured by this tool in a process of its own in the same session"
    for S in counts:
        sections = torch.stack([song[:, s * a.samples:(s + 1) * a.samples] for s in range(S)]).contiguous()
        args = (sections, profile, console, loss)
        mine, single, batch = [], [], []
        for _ in range(a.rounds):  # alternating within a round
            if not a.baseline_only:
                torch.manual_seed(1)
                mine.append(timed(sections_loop, args, a.warmup, a.iters))
            if given is None:
                if S == 1:
                    torch.manual_seed(1)
                    single.append(timed(single_loop, args, a.warmup, a.iters))
                torch.manual_seed(1)
                batch.append(timed(batch_loop, args, a.warmup, a.iters))
        if given is None:
            result["baseline"].append(dict(S=S, single=stat(single) if single else None, batch=stat(batch),
                                           launches_single=counted(single_loop, args) if S == 1 else None,
                                           launches_batch=counted(batch_loop, args)))
            print(f"S={S}: optimize_batch {result['baseline'][-1]['batch']['median']:.3f} ms per iteration", flush=True)
        if not a.baseline_only:
            result["rows"].append(dict(S=S, sections=stat(mine), launches_sections=counted(sections_loop, args)))
            print(f"S={S}: optimize_sections {result['rows'][-1]['sections']['median']:.3f} ms per iteration", flush=True)
    if a.out:
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
