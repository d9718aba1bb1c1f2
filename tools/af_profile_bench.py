"""AudioFeatureLoss against a feature profile, timed beside the paired-tensor path; writes profiles/af_profile.md.

    python tools/af_profile_bench.py [--reps 20] [--rounds 5] [--opt-iters 30] [--out profiles/af_profile.md]

* Loss forward + backward at (1, 2, 524288) and (8, 2, 262144): HIP events around ``reps`` back-to-back repetitions after a warm-up of the
  same, the two paths alternating within a round; median over the rounds, with the spread.  The paired path is untouched by the profile
  work, i.e. it is the baseline of the same session on the same machine.  ``profile()`` alone is timed the same way.
* ``mst.online.optimize`` per iteration at T = 16, N = 524288 as tools/online_bench.py times it (a host clock from iteration ``warmup`` to
  a device synchronise after the last one, ``validate="deferred"``): an equal-length tensor reference against ``loss.profile(ref)``.
* The strip plan of each path: ``plan()`` restates ``af_groups`` of csrc/mst_af.hip (frames cut into G strips per (signal, half) unit,
  512 co-resident workgroups).

Needs the MI355X: there is no CPU path.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-mst_amd"), os.path.join(ROOT, "diff-mst_amd", "standalone")]
import torch  # noqa: E402

from mst.loss import AF_KEYS, AudioFeatureLoss  # noqa: E402
from mst.modules import AdvancedMixConsole  # noqa: E402
from mst.online import optimize  # noqa: E402

AF_WEIGHTS = [0.1, 0.001, 1.0, 1.0, 0.1]
ONLINE_WEIGHTS = [0.1, 0.001, 1.0, 1.0, 1.0]  # tools/online_bench.py
SLOTS = 512


def plan(n, units):
    """(frames, strips G, rounds, longest strip) as af_groups chooses them for ``units`` (signal, half) units."""
    frames = 1 + n // 8192
    best = None
    for g in range(1, frames + 1):
        rounds, length = -(-g * units // SLOTS), -(-frames // g)
        cost = rounds * length * 1024 + g
        if best is None or cost < best[0]:
            best = (cost, g, rounds, length)
    return (frames,) + best[1:]


def events_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def loss_rows(bs, n, reps, rounds, dev):
    torch.manual_seed(bs + n)
    f = AudioFeatureLoss(AF_WEIGHTS, 44100)
    x = (0.2 * torch.randn(bs, 2, n)).to(dev).requires_grad_(True)
    y = (0.3 * torch.randn(bs, 2, n)).to(dev)
    prof = f.profile(y)

    def step(target):
        def run():
            x.grad = None
            ld = f(x, target)
            torch.autograd.backward([ld[k] for k in AF_KEYS], [torch.ones_like(ld[k]) for k in AF_KEYS])
        return run

    def forward(target):
        def run():
            with torch.no_grad():
                f(x, target)
        return run

    fns = {"paired fwd+bwd": step(y), "profile fwd+bwd": step(prof), "paired fwd": forward(y), "profile fwd": forward(prof),
           "profile() of the target": lambda: f.profile(y)}
    for fn in fns.values():
        events_ms(fn, 5)  # warm-up: code objects, tables, the allocator's blocks
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():  # alternating within a round
            ms[k].append(events_ms(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def optimize_rows(n_tracks, n, warmup, iters, rounds, dev):
    torch.manual_seed(0)
    tracks = (0.1 * torch.randn(n_tracks, n)).to(dev)
    f = AudioFeatureLoss(ONLINE_WEIGHTS, 44100)
    console = AdvancedMixConsole(44100, validate="deferred")
    with torch.no_grad():
        ref = AdvancedMixConsole(44100)(tracks[None], *(torch.rand(s, device=dev) * 0.5 + 0.25 for s in ((1, n_tracks, 27), (1, 25), (1, 26))),
                                        use_fx_bus=False)[1][0].clone()
    refs = {"tensor reference (paired)": ref, "loss.profile(ref)": f.profile(ref[None])}

    def timed(target):
        t0 = []

        def mark(k, view):
            if k == warmup:
                torch.cuda.synchronize()
                t0.append(time.perf_counter())

        torch.manual_seed(1)
        history = optimize(tracks, target, console, f, lr=1e-3, n_iters=warmup + iters, callback=mark)[7]["loss"]
        torch.cuda.synchronize()
        assert all(v == v for v in history), "a loss was NaN"
        return (time.perf_counter() - t0[0]) * 1e3 / iters

    ms = {k: [] for k in refs}
    for _ in range(rounds):
        for k, target in refs.items():
            ms[k].append(timed(target))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--opt-warmup", type=int, default=5)
    ap.add_argument("--opt-iters", type=int, default=30)
    ap.add_argument("--opt-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "af_profile.md"))
    a = ap.parse_args()
    if a.rounds < 3 or a.opt_rounds < 3:
        raise SystemExit("at least three rounds")
    if not torch.cuda.is_available():
        raise SystemExit("af_profile_bench needs the MI355X")
    dev = torch.device("cuda:0")
    lines = ["# AudioFeatureLoss against a feature profile", "",
             f"`tools/af_profile_bench.py` on {torch.cuda.get_device_name(0)}: HIP events around {a.reps} back-to-back repetitions, the paths "
             f"alternating within a round, median of {a.rounds} rounds (min - max).  The paired path is the parent commit's, untouched.", ""]
    for bs, n in ((1, 524288), (8, 262144)):
        rows = loss_rows(bs, n, a.reps, a.rounds, dev)
        pf, pg = plan(n, 8 * bs), plan(n, 4 * bs)
        lines += [f"## loss at ({bs}, 2, {n})", "",
                  f"Strip plan (frames, strips per unit, rounds, longest strip): paired {pf} over {8 * bs} (signal, half) units; "
                  f"profile {pg} over {4 * bs} units.", "", "| call | ms | min - max |", "|---|---|---|"]
        for k, (med, lo, hi) in rows.items():
            lines.append(f"| {k} | {med:.4f} | {lo:.4f} - {hi:.4f} |")
            print(f"({bs}, 2, {n}) {k}: {med:.4f} ms ({lo:.4f} - {hi:.4f})", flush=True)
        lines += ["", f"profile / paired, forward + backward: {rows['profile fwd+bwd'][0] / rows['paired fwd+bwd'][0]:.3f}; "
                      f"forward alone: {rows['profile fwd'][0] / rows['paired fwd'][0]:.3f}", ""]
    T, N = 16, 524288
    rows = optimize_rows(T, N, a.opt_warmup, a.opt_iters, a.opt_rounds, dev)
    lines += [f"## optimize at T = {T}, N = {N}", "",
              f"Host clock over iterations {a.opt_warmup}..{a.opt_warmup + a.opt_iters - 1} of a run, ending in a device synchronise, "
              f"`validate=\"deferred\"`; median of {a.opt_rounds} runs (min - max).", "", "| reference | ms / iteration | min - max |", "|---|---|---|"]
    for k, (med, lo, hi) in rows.items():
        lines.append(f"| {k} | {med:.3f} | {lo:.3f} - {hi:.3f} |")
        print(f"optimize T={T} N={N} {k}: {med:.3f} ms / iteration ({lo:.3f} - {hi:.3f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
