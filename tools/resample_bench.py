"""Developer timing of the device resampler (not the contract bench; see bench.py).

  python tools/resample_bench.py kernels   mst.utils.resample against the dense formulation torchaudio would launch (the strided
                                           conv1d of tests/resample_ref.py, in torch on the same GPU): 48000 -> 44100 and
                                           44100 -> 48000 at 8 x 524288 and 16 x 10584000, HIP events, alternating, and the adjoint
  python tools/resample_bench.py trace     a few calls of each shape and nothing else: run it under
                                           `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/resample_bench.py trace`
  python tools/resample_bench.py e2e       run_diffmst on the fixture recipe with the tracks taken as 48 kHz material
                                           (track_sample_rate=48000) against the same call on tracks converted beforehand
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

dev = torch.device("cuda:0")
SHAPES = ((8, 524288), (16, 10584000))
RATIOS = ((48000, 44100), (44100, 48000))


def spread(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), n=len(v))


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernels(reps=20):
    import resample_ref as R

    out = {}
    for orig, new in RATIOS:
        for rows, n in SHAPES:
            x = 0.1 * torch.randn(rows, n, device=dev)
            n_out = R.out_samples(n, orig, new)
            g = torch.randn(rows, n_out, device=dev)
            xg = x.clone().requires_grad_()
            yg = U.resample(xg, orig, new)
            calls = {
                "hip": lambda: U.resample(x, orig, new),
                "dense_conv1d": lambda: R.resample(x, orig, new, torch.float32),
                "hip_adjoint": lambda: torch.autograd.grad(yg, xg, g, retain_graph=True),
            }
            for fn in calls.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in calls}
            for _ in range(reps):  # alternating
                for k, fn in calls.items():
                    times[k].append(event_time(fn))
            moved = 4.0 * rows * (n + n_out)
            res = {k: spread(v) for k, v in times.items()}
            for k in ("hip", "hip_adjoint"):
                res[k]["moved_MB"] = moved / 1e6
                res[k]["share_of_8TBps"] = moved / (res[k]["median_ms"] * 1e-3) / 8e12
            res["dense_over_hip"] = res["dense_conv1d"]["median_ms"] / res["hip"]["median_ms"]
            res["max_abs_diff_hip_vs_dense"] = float((U.resample(x, orig, new) - R.resample(x, orig, new, torch.float32)).abs().max())
            out[f"{orig}->{new} {rows}x{n}"] = res
            del x, g, xg, yg
            torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))


def trace():
    for orig, new in RATIOS:
        for rows, n in SHAPES:
            x = (0.1 * torch.randn(rows, n, device=dev)).requires_grad_()
            for _ in range(5):
                y = U.resample(x, orig, new)
                y.backward(torch.ones_like(y))
                x.grad = None
            torch.cuda.synchronize()
            del x, y
            torch.cuda.empty_cache()


def e2e(reps=12):
    import numpy as np

    from mst.modules import AdvancedMixConsole
    from util import StubModel

    g = np.load(os.path.join(ROOT, "tests", "golden", "run_diffmst.npz"))
    T, n = (int(v) for v in g["shape"])
    torch.manual_seed(int(g["seed_tracks"]))
    tracks = (0.05 * torch.randn(1, T, n) * torch.tensor([1.0, 0.3, 2.0, 1e-6, 0.7]).view(1, T, 1)).half().float().to(dev)
    ref = (0.2 * torch.randn(1, 2, int(g["ref_len"]))).to(dev)
    model = StubModel(seed=int(g["seed_model"])).to(dev)
    console = AdvancedMixConsole(44100)
    kw = dict(track_start_idx=int(g["track_start_idx"]), ref_start_idx=int(g["ref_start_idx"]), loudness_fn="device")
    converted = U.resample(tracks, 48000, 44100)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    calls = {
        "tracks_48k_converted_in_the_call": lambda: U.run_diffmst(tracks, ref, model, console, track_sample_rate=48000, **kw),
        "tracks_converted_beforehand": lambda: U.run_diffmst(converted, ref, model, console, **kw),
        "resample_alone": lambda: U.resample(tracks, 48000, 44100),
    }
    for fn in calls.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in calls}
    for _ in range(reps):  # alternating
        for k, fn in calls.items():
            times[k].append(timed(fn))
    print(json.dumps({"tracks": [T, n], "tracks_at_44100": list(converted.shape[1:]), **{k: spread(v) for k, v in times.items()}}, indent=1))


if __name__ == "__main__":
    {"kernels": kernels, "trace": trace, "e2e": e2e}[sys.argv[1]]()
