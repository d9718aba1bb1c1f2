"""The section picker's rule (``mst_pick_sections``, include/diffmst_hip.h) restated in numpy, and the call through a bound library
that the simulator and the GPU tests share.

TEST INFRASTRUCTURE: numpy only (and torch for the call).
"""
import numpy as np
import torch


def pick_sections(track_lufs, mix_lufs, track_floor, mix_floor, count, min_gap):
    """-> (windows (count,) int32 with -1 where no candidate was left, active (count, T) uint8, covered (T,) uint8)"""
    track_lufs, mix_lufs = np.asarray(track_lufs, np.float32), np.asarray(mix_lufs, np.float32)
    T, NW = track_lufs.shape
    with np.errstate(invalid="ignore"):
        active = track_lufs >= np.asarray(track_floor, np.float32)[:, None]
        eligible = (mix_lufs >= np.float32(mix_floor)) & active.any(axis=0)
    covered, chosen = np.zeros(T, bool), []
    windows, rows = np.full(count, -1, np.int32), np.zeros((count, T), np.uint8)
    act = active.sum(axis=0)
    for r in range(count):
        cand = [w for w in range(NW) if eligible[w] and all(abs(w - c) >= min_gap for c in chosen)]
        if not cand:
            break
        new = (active & ~covered[:, None]).sum(axis=0)
        w = max(cand, key=lambda w: (int(new[w]), int(act[w]), float(mix_lufs[w]), -w))
        chosen.append(w)
        covered |= active[:, w]
        windows[r], rows[r] = w, active[:, w]
    return windows, rows, covered.astype(np.uint8)


def call_picker(L, track_lufs, mix_lufs, track_floor, mix_floor, count, min_gap):
    """fp32 tensors on one device -> (windows, active, covered) as numpy arrays.  The outputs start as garbage: every element must be
    written."""
    T, NW = track_lufs.shape
    dev = track_lufs.device
    windows = torch.full((count,), -77, dtype=torch.int32, device=dev)
    active = torch.full((count, T), 0xAA, dtype=torch.uint8, device=dev)
    covered = torch.full((T,), 0xAA, dtype=torch.uint8, device=dev)
    L.mst_pick_sections(track_lufs.contiguous(), mix_lufs.contiguous(), track_floor.contiguous(), float(mix_floor), T, NW, count, min_gap,
                        windows, active, covered, None)
    return windows.cpu().numpy(), active.cpu().numpy(), covered.cpu().numpy()


def random_tables(T, NW, seed, levels=12):
    """Loudness tables with many exact ties (a few distinct levels), silent entries (-inf), NaN entries and stretches where nothing plays:
    -> (track_lufs (T, NW), mix_lufs (NW), track_floor (T), mix_floor) float32 numpy."""
    rng = np.random.default_rng(seed)
    track = -60.0 + 3.0 * rng.integers(0, levels, size=(T, NW)).astype(np.float32)   # floors at -48: a third of them below
    on = rng.random((T, 1)) < 0.5                                                    # half of the tracks play in one stretch only
    lo = rng.integers(0, NW, size=(T, 1))
    span = np.abs(np.arange(NW)[None, :] - lo) <= max(1, NW // 8)
    track = np.where(on & ~span, -np.inf, track).astype(np.float32)
    track[rng.random((T, NW)) < 0.02] = np.nan
    mix = (-55.0 + 2.0 * rng.integers(0, levels, size=NW)).astype(np.float32)
    mix[rng.random(NW) < 0.02] = np.nan
    floor = (-48.0 + 3.0 * rng.integers(-1, 2, size=T)).astype(np.float32)
    return track, mix, floor, np.float32(-48.0)
