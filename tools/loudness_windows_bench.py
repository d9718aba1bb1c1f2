"""Developer timing of the windowed loudness and the section picker (not the contract bench; see bench.py).

  python tools/loudness_windows_bench.py song [ROWS SECONDS]
        17 rows x 240 s at 44100 Hz (16 tracks and their sum), windows of 524288 samples every 0.1 s: mst.utils.windowed_loudness and
        mst.online.pick_sections against the only route there was before - mst.utils.integrated_loudness over an as_strided view of
        the same overlapping windows, one call per row (a call takes 13107 rows at most).  HIP events for the device calls, a host
        clock around a synchronise for pick_sections (it reads the picked windows back).  Also how far the two routes are apart.
  python tools/loudness_windows_bench.py parent PATH_TO_PARENT_LIBRARY
        mst_loudness_integrated at 16 x 262144 through this build and through a build of the parent commit (make -C diff-mst_amd/csrc
        OUT=... BUILD=... in a checkout of it), alternating in one process, and whether the two write the same bits there and on the
        shapes of tests/test_loudness_hostsim.py.
"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "diff-mst_amd"), os.path.join(ROOT, "diff-mst_amd", "standalone"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from mst import _cabi, _hip  # noqa: E402
from mst import utils as U  # noqa: E402
from mst.online import pick_sections  # noqa: E402

dev = torch.device("cuda:0")
RATE, LENGTH, HOP = 44100, 524288, 4410


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


def song(rows=17, seconds=240):
    n = seconds * RATE
    g = torch.Generator(device=dev).manual_seed(0)
    tracks = 0.05 * torch.randn(rows - 1, n, generator=g, device=dev)
    for t in range(rows - 1):  # every track rests for a sixth of the song, somewhere else each
        lo = (t * n) // (rows - 1)
        tracks[t, lo:lo + n // 6] = 0.0
    x = torch.cat((tracks, tracks.sum(0, keepdim=True))).unsqueeze(1)  # (rows, 1, n)
    W, H, starts = U.loudness_window_grid(n, LENGTH, HOP, RATE)
    fit = sum(1 for s in starts if s + LENGTH <= n)  # a window's blocks end up to 0.1 s before its LENGTH samples do: the last crops may not fit

    def new():
        return U.windowed_loudness(x, LENGTH, HOP, RATE)[0]

    def old():
        # window w of row r starts at r n + w HOP: a (NW, 1, LENGTH) view per row, metered as NW crops
        return torch.stack([U.integrated_loudness(torch.as_strided(x[r], (fit, 1, LENGTH), (HOP, n, 1)), RATE) for r in range(rows)])

    out = dict(rows=rows, n_samples=n, length=LENGTH, hop=HOP, window_blocks=W, windows=len(starts), baseline_crops=fit,
               baseline_blocks_per_crop=_hip.lib().mst_loudness_num_blocks(LENGTH, RATE))
    a, b = new()[:, :fit], old()
    torch.cuda.synchronize()
    fin = torch.isfinite(a) & torch.isfinite(b)
    out["finite_windows"] = int(fin.sum())
    out["max_abs_difference_LU"] = float((a - b)[fin].abs().max())
    out["median_abs_difference_LU"] = float((a - b)[fin].abs().median())
    new_ts, old_ts = [], []
    for _ in range(3):  # alternating
        new_ts += events(new, 5)
        old_ts += events(old, 1)
    out["windowed_loudness"] = spread(new_ts)
    out["integrated_loudness_on_crops"] = spread(old_ts)
    out["ratio_of_medians"] = out["integrated_loudness_on_crops"]["median_ms"] / out["windowed_loudness"]["median_ms"]
    pick = pick_sections(tracks, LENGTH, 8)  # warm-up
    ts = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pick = pick_sections(tracks, LENGTH, 8)
        ts.append(1e3 * (time.perf_counter() - t0))  # ends in the host read of the picked windows
    out["pick_sections_count_8"] = spread(ts)
    out["picked_starts"] = pick.starts
    out["tracks_covered"] = int(pick.covered.sum())
    # the picker launch alone, at its limits: 256 tracks x 4092 windows, 64 sections
    lib = _hip.lib()
    tl = -60.0 + 30.0 * torch.rand(256, 4092, device=dev)
    ml, fl = -40.0 + 30.0 * torch.rand(4092, device=dev), torch.full((256,), -48.0, device=dev)
    w, act, cov = torch.empty(64, dtype=torch.int32, device=dev), torch.empty(64, 256, dtype=torch.uint8, device=dev), torch.empty(256, dtype=torch.uint8, device=dev)
    call = lambda: lib.mst_pick_sections(tl, ml, fl, -48.0, 256, 4092, 64, 7, w, act, cov, _hip.current_stream_ptr(dev))
    call()
    out["mst_pick_sections_256x4092x64"] = spread(events(call, 20))
    print(json.dumps(out, indent=1))


def bind_what_it_has(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in _cabi.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes = args
            if res is _cabi.STATUS:
                fn.restype, fn.errcheck = ctypes.c_int, _cabi._raise_on_status
            else:
                fn.restype = res
    return lib


def parent(path):
    import loudness_ref as R
    from test_loudness_hostsim import CASES

    libs = {"this": _hip.lib(), "parent": bind_what_it_has(path)}
    assert not hasattr(libs["parent"], "mst_loudness_windows"), "that is not a build of the parent commit"

    def meter(lib, x, rate):
        rows, chs, n = x.shape
        nbytes, nb = lib.mst_loudness_workspace_bytes(rows, chs, n, rate), lib.mst_loudness_num_blocks(n, rate)
        tables = torch.empty(lib.mst_loudness_tables_bytes(rate), dtype=torch.uint8, device=dev)
        lib.mst_loudness_init_tables(rate, tables, _hip.current_stream_ptr(dev))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        lufs, blocks = torch.empty(rows, device=dev), torch.empty(rows, nb, device=dev)
        run = lambda: lib.mst_loudness_integrated(x, rows, chs, n, x.stride(0), x.stride(1), rate, tables, lufs, blocks, ws, nbytes,
                                                  _hip.current_stream_ptr(dev))
        run()
        torch.cuda.synchronize()
        return run, lufs, blocks

    out = {"bit_identical": {}}
    shapes = [(44100, 16, 1, 262144, 11)] + [(rate, rows, chs, n, seed) for rate, rows, chs, n, _, seed in CASES]
    for rate, rows, chs, n, seed in shapes:
        x = torch.from_numpy(R.level_step_noise(rows, chs, n, seed)).to(dev)
        (_, la, ba), (_, lb, bb) = meter(libs["this"], x, rate), meter(libs["parent"], x, rate)
        out["bit_identical"][f"{rate}:{rows}x{chs}x{n}"] = bool(torch.equal(la.view(torch.int32), lb.view(torch.int32)) and
                                                               torch.equal(ba.view(torch.int32), bb.view(torch.int32)))
    x = 0.1 * torch.randn(16, 1, 262144, device=dev)
    runs = {k: meter(lib, x, 44100)[0] for k, lib in libs.items()}
    times = {k: [] for k in runs}
    for _ in range(5):  # alternating
        for k, run in runs.items():
            times[k] += events(run, 20)
    out["mst_loudness_integrated_16x262144"] = {k: spread(v) for k, v in times.items()}
    print(json.dumps(out, indent=1))
    assert all(out["bit_identical"].values())


if __name__ == "__main__":
    if sys.argv[1] == "song":
        song(*(int(v) for v in sys.argv[2:4]))
    else:
        parent(sys.argv[2])
