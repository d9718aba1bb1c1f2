"""Developer timing of the delivery meter (not the contract bench; see bench.py).

  python tools/metering_bench.py all
        true_peak at 16 x 10584000 (4-minute stems, one channel each) and at 2 x 2 x 524288 against the only device route there was
        before - resample(x, r, 4 r).abs().amax() - and against reading the input once at the achievable HBM rate; meter_report at
        2 x 2 x 10584000 against its parts called one by one; loudness_range against integrated_loudness.  HIP events around each
        call, the routes alternating in one process; medians, spread and the number of launches of each route.
  python tools/metering_bench.py kernel
        the true-peak launches alone at 16 x 10584000, five times: the run to put under a counter collection of its own.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-mst_amd"), os.path.join(ROOT, "diff-mst_amd", "standalone")]
import torch  # noqa: E402

from mst import utils as U  # noqa: E402

dev = torch.device("cuda:0")
RATE = 44100
HBM_ACHIEVABLE_GBS = 6300.0  # a float4 copy on this part (8000 is the specification; profiles/round4_hbm_calibration.md read 4.5 - 6.6)


def spread(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), n=len(v))


def events(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def alternate(routes, rounds, reps):
    for fn in routes.values():  # warm-up: tables, allocator
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k] += events(fn, reps)
    return {k: spread(v) for k, v in times.items()}


def peak_routes(x):
    rows = x.reshape(-1, x.shape[-1])
    return {"true_peak": lambda: U.true_peak(x, RATE),
            "resample_abs_amax": lambda: U.resample(rows, RATE, 4 * RATE).abs().amax(dim=-1)}


def main():
    out = {}
    g = torch.Generator(device=dev).manual_seed(0)
    stems = 0.1 * torch.randn(16, 1, 240 * RATE, generator=g, device=dev)
    small = 0.1 * torch.randn(2, 2, 524288, generator=g, device=dev)
    for name, x in (("16x1x10584000", stems), ("2x2x524288", small)):
        r = alternate(peak_routes(x), 3, 5)
        nbytes = x.numel() * 4
        r["input_bytes"] = nbytes
        r["read_once_ms_at_%d_GBs" % HBM_ACHIEVABLE_GBS] = nbytes / (HBM_ACHIEVABLE_GBS * 1e6)
        r["true_peak_GBs_of_input"] = nbytes / (r["true_peak"]["median_ms"] * 1e6)
        r["ratio_of_medians"] = r["resample_abs_amax"]["median_ms"] / r["true_peak"]["median_ms"]
        r["launches"] = {"true_peak": "2 kernels + 1 elementwise log10", "resample_abs_amax": "1 kernel + abs + amax (writes 4x the input)"}
        a = U.true_peak(x, RATE)
        b = 20.0 * torch.log10(U.resample(x.reshape(-1, x.shape[-1]), RATE, 4 * RATE).abs().amax(dim=-1)).view(x.shape[0], -1).amax(dim=1)
        r["max_abs_difference_dB_between_the_routes"] = float((a - b).abs().max())
        out["true_peak_" + name] = r
    song = 0.1 * torch.randn(2, 2, 240 * RATE, generator=g, device=dev)

    def parts():
        U.integrated_loudness(song, RATE, return_blocks=True)
        U.loudness_range(song, RATE)
        U.short_term_loudness(song, sample_rate=RATE)
        U.true_peak(song, RATE)
        song.abs().amax(dim=(1, 2))

    out["meter_report_2x2x10584000"] = alternate({"meter_report": lambda: U.meter_report(song, RATE), "its_parts_one_by_one": parts}, 3, 5)
    out["meter_report_2x2x10584000"]["launches"] = {"meter_report": "5 meter + 2 true-peak kernels + 4 elementwise", "its_parts_one_by_one": "4 + 5 + 5 + 2 kernels + elementwise"}
    out["loudness_range_2x2x10584000"] = alternate({"loudness_range": lambda: U.loudness_range(song, RATE),
                                                    "loudness_range_hop_0.1s": lambda: U.loudness_range(song, RATE, hop=RATE // 10),
                                                    "integrated_loudness": lambda: U.integrated_loudness(song, RATE)}, 3, 5)
    print(json.dumps(out, indent=1))


def kernel():
    x = 0.1 * torch.randn(16, 1, 240 * RATE, device=dev)
    for _ in range(5):
        U.true_peak(x, RATE)
    torch.cuda.synchronize()


if __name__ == "__main__":
    kernel() if sys.argv[1:] == ["kernel"] else main()
