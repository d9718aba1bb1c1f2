"""Developer timing of the device loudness meter (not the contract bench; see bench.py).

  python tools/loudness_bench.py kernels   meter at 16 x 262144 and 512 x 131072 (HIP events), and a few console fwd+bwd steps at
                                           cfg #2 so that a kernel trace of this run shows k_cascade_zsin next to the k_loud_* kernels
  python tools/loudness_bench.py e2e       run_diffmst on the fixture recipe: loudness_fn="device" against the host path with the
                                           float64 restatement (tests/loudness_ref.py) injected, alternating, host clock around a
                                           device synchronise; the normalisation stage alone and the whole call
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-mst_amd"), os.path.join(ROOT, "diff-mst_amd", "standalone"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from mst import utils as U  # noqa: E402
from mst.modules import AdvancedMixConsole  # noqa: E402

dev = torch.device("cuda:0")


def spread(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), n=len(v))


def kernels():
    out = {}
    for rows, n in ((16, 262144), (512, 131072)):
        x = 0.1 * torch.randn(rows, 1, n, device=dev)
        for _ in range(3):
            U.integrated_loudness(x)
        torch.cuda.synchronize()
        ts = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            U.integrated_loudness(x)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        s = spread(ts)
        s["input_MB"] = rows * n * 4 / 1e6
        s["share_of_8TBps"] = rows * n * 4 / (s["median_ms"] * 1e-3) / 8e12
        out[f"meter_{rows}x{n}"] = s
        ts = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            U.loudness_normalize(x, -48.0, floor_lufs=-80.0)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        out[f"meter_and_normalize_{rows}x{n}"] = spread(ts)
        del x
    # console fwd+bwd at cfg #2 (tools/quick_bench.py): the 12-state EQ pass of 64 rows x 262144 in the same trace
    bs, T, n = 8, 8, 262144
    c = AdvancedMixConsole(44100, materialize_mixed_tracks=False, validate="deferred")
    tracks = 0.1 * torch.randn(bs, T, n, device=dev)
    tp = torch.rand(bs, T, 27, device=dev, requires_grad=True)
    fp = torch.rand(bs, 25, device=dev)
    mp = torch.rand(bs, 26, device=dev, requires_grad=True)
    g = torch.randn(bs, 2, n, device=dev)
    for _ in range(5):
        tp.grad = None
        mp.grad = None
        _, mix, *_ = c(tracks, tp, fp, mp, use_fx_bus=False)
        mix.backward(g)
    torch.cuda.synchronize()
    print(json.dumps(out, indent=1))


def e2e(reps=12):
    import numpy as np

    import loudness_ref as R
    from util import StubModel

    g = np.load(os.path.join(ROOT, "tests", "golden", "run_diffmst.npz"))
    T, n = (int(v) for v in g["shape"])
    torch.manual_seed(int(g["seed_tracks"]))
    tracks = (0.05 * torch.randn(1, T, n) * torch.tensor([1.0, 0.3, 2.0, 1e-6, 0.7]).view(1, T, 1)).half().float()
    ref = 0.2 * torch.randn(1, 2, int(g["ref_len"]))
    model = StubModel(seed=int(g["seed_model"])).to(dev)
    console = AdvancedMixConsole(44100)
    start = int(g["track_start_idx"])
    kw = dict(track_start_idx=start, ref_start_idx=int(g["ref_start_idx"]))
    host_meter = lambda a: R.integrated_loudness(a, 44100)
    analysis = tracks[..., start:start + U.ANALYSIS_LEN]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    calls = {
        "stage_device": lambda: U._normalize_tracks_on_device(tracks, n, start, dev, False),
        "stage_host_f64_restatement": lambda: U._normalize_tracks_on_host(tracks, analysis, host_meter, dev, False),
        "whole_device": lambda: U.run_diffmst(tracks, ref, model, console, loudness_fn="device", **kw),
        "whole_host_f64_restatement": lambda: U.run_diffmst(tracks, ref, model, console, loudness_fn=host_meter, **kw),
    }
    for fn in calls.values():  # warm-up
        for _ in range(2):
            fn()
    times = {k: [] for k in calls}
    for _ in range(reps):  # alternating
        for k, fn in calls.items():
            times[k].append(timed(fn))
    dev_tracks = tracks.to(dev)
    calls_dev = {"stage_device_tracks_already_on_device": lambda: U._normalize_tracks_on_device(dev_tracks, n, start, dev, False)}
    for k, fn in calls_dev.items():
        fn()
        times[k] = [timed(fn) for _ in range(reps)]
    print(json.dumps({"tracks": [T, n], **{k: spread(v) for k, v in times.items()}}, indent=1))


if __name__ == "__main__":
    {"kernels": kernels, "e2e": e2e}[sys.argv[1]]()
