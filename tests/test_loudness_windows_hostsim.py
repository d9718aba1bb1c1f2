"""``mst_loudness_windows`` (diff-mst_amd/csrc/mst_loudness.hip) on the host simulator, against (1) the float64 restatement of the
windowed loudness (tests/loudness_windows_ref.py: the signal filtered once, every window gated on its own), (2) the closed-form level
of a stationary sine, (3) its bit-level properties and its agreement with ``mst_loudness_integrated``, (4) what it refuses.  The
bounds are the meter's own (tests/test_loudness_hostsim.py)."""
import math

import numpy as np
import pytest
import torch

import loudness_ref as R
import loudness_windows_ref as WR
from test_loudness_hostsim import CLOSED_FORM_TOL_LU, FP32_ALLOWANCE_LU, GATE_MARGIN_LU, lib, meter, tables  # noqa: F401


def blocks_wholly_inside(n, rate, lo_frac, hi_frac):
    """Complete gating blocks that lie inside [int(lo_frac n), int(hi_frac n))."""
    lo, hi = int(lo_frac * n), int(hi_frac * n)
    return [j for j in range(WR.num_complete_blocks(n, rate)) if R.block_bounds(j, rate)[0] >= lo and R.block_bounds(j, rate)[1] <= hi]


# ---- 1. against the restatement -------------------------------------------------------------------------------------------------
WINDOW_CASES = [
    # rate, rows, channels, n, W, H, (front pad, back pad), seed, what the restatement's windows must show:
    # a window that loses a block to the relative gate / to the absolute gate / that lies wholly in the 1e-6 stretch
    (44100, 3, 2, 70000, 4, 1, (8, 120), 12, True, True, False),
    (48000, 2, 1, 70001, 3, 2, (3, 2), 13, True, True, False),
    (44100, 1, 1, 262144, 11, 1, (0, 0), 11, True, True, True),
    (44100, 1, 5, 17640 + 4 * 4410, 1, 1, (0, 0), 14, False, False, False),  # one-block windows, all five channel weights
    (44100, 2, 2, 70000, None, 1, (0, 0), 16, True, True, False),            # W = NB: one window of every complete block
]


@pytest.mark.parametrize("rate,rows,chs,n,W,H,pad,seed,loses_rel,loses_abs,silent", WINDOW_CASES)
def test_windows_match_the_float64_restatement(lib, rate, rows, chs, n, W, H, pad, seed, loses_rel, loses_abs, silent):
    nb = WR.num_complete_blocks(n, rate)
    W = nb if W is None else W
    x = R.level_step_noise(rows, chs, n, seed)
    ref = [WR.windowed_loudness(x[r], rate, W, H) for r in range(rows)]
    nw = WR.num_windows(nb, W, H)
    # the pre-check runs on the restatement alone, for every window: no block of a window may sit closer to one of its gates
    seen_rel = seen_abs = False
    for r in range(rows):
        assert len(ref[r][0]) == nw
        for w, (l, a, f) in enumerate(ref[r][1]):
            m_rel, m_abs = WR.window_margins(l)
            assert m_rel > GATE_MARGIN_LU and m_abs > GATE_MARGIN_LU, f"row {r} window {w}: a block sits on a gate, change the seed"
            seen_rel |= len(f) < len(a)
            seen_abs |= len(a) < W
    assert seen_rel == loses_rel and seen_abs == loses_abs
    full = torch.zeros(rows, chs, pad[0] + n + pad[1])
    full[..., pad[0]:pad[0] + n] = torch.from_numpy(x)
    view = full[..., pad[0]:pad[0] + n]
    assert pad == (0, 0) or not view.is_contiguous()
    assert WR.count_windows(lib, n, rate, W, H) == nw
    got, _ = WR.call_windows(lib, view, rate, tables(lib, rate), W, H)
    got = got.double().numpy()
    _, blocks = meter(lib, view, rate)  # the kernels' own block loudness: the gate sets they formed
    worst = 0.0
    for r in range(rows):
        want = ref[r][0]
        assert np.array_equal(np.isfinite(got[r]), np.isfinite(want)) and np.all(np.isneginf(got[r][~np.isfinite(want)]))
        fin = np.isfinite(want)
        if fin.any():
            worst = max(worst, float(np.max(np.abs(got[r][fin] - want[fin]))))
        for w, (_, a, f) in enumerate(ref[r][1]):
            assert WR.kernel_gate_sets(blocks[r], W, H, w) == (a, f), f"row {r} window {w}: gate sets differ"
    print(f"\n[{rate} Hz {rows}x{chs}x{n} W={W} H={H}] {nw} windows, |L - L_f64| = {worst:.3e} LU (bound {FP32_ALLOWANCE_LU:.1e})")
    assert worst <= FP32_ALLOWANCE_LU
    inside = blocks_wholly_inside(n, rate, 0.55, 0.9)
    quiet = [w for w in range(nw) if all(j in inside for j in range(w * H, w * H + W))]
    assert bool(quiet) == silent
    for r in range(rows):
        assert np.all(np.isneginf(got[r][quiet]))


# ---- 2. closed form -------------------------------------------------------------------------------------------------------------
def test_full_scale_sine_windows_match_the_closed_form(lib):
    rate, freq = 44100, 997.0
    n = 10 * rate
    x = np.sin(2.0 * math.pi * freq * np.arange(n) / rate)
    closed = -0.691 + 10.0 * math.log10(0.5 * R.response_sq(rate, freq))
    got, _ = WR.call_windows(lib, torch.from_numpy(x.astype(np.float32)).view(1, 1, n), rate, tables(lib, rate), 27, 1)
    got = got.double().numpy()[0]
    assert len(got) == 97 - 27 + 1
    print(f"\n[sine windows] closed form {closed:.6f}, worst window {np.max(np.abs(got - closed)):.3e} LU (bound {CLOSED_FORM_TOL_LU:.2e})")
    assert np.max(np.abs(got - closed)) <= CLOSED_FORM_TOL_LU


# ---- 3. bit-level properties ------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int32)


def test_hop_nan_workspace_and_repeat_are_bit_identical(lib):
    rate, n = 44100, 70000
    x = torch.from_numpy(R.level_step_noise(2, 2, n, 51))
    t = tables(lib, rate)
    one, lufs = WR.call_windows(lib, x, rate, t, 3, 1)
    again, _ = WR.call_windows(lib, x, rate, t, 3, 1, want_lufs=False)
    zeros, _ = WR.call_windows(lib, x, rate, t, 3, 1, fill=0.0)
    assert torch.equal(bits(one), bits(again)) and torch.equal(bits(one), bits(zeros)) and not torch.isnan(one).any()
    for k in (2, 3, 5):
        hop, _ = WR.call_windows(lib, x, rate, t, 3, k)
        assert torch.equal(bits(hop), bits(one[:, ::k]))
    # the optional whole-signal output is the meter's, bit for bit (70000 samples: the meter also counts a clipped partial block)
    nbytes = lib.mst_loudness_workspace_bytes(2, 2, n, rate)
    ws = torch.full((nbytes // 8 + 1,), float("nan"), dtype=torch.float64)
    whole = torch.full((2,), float("nan"))
    lib.mst_loudness_integrated(x, 2, 2, n, x.stride(0), x.stride(1), rate, t, whole, None, ws, nbytes, None)
    assert torch.equal(bits(lufs), bits(whole))


@pytest.mark.parametrize("m,rows,chs", [(0, 3, 2), (1, 3, 2), (7, 3, 2), (70, 1, 1)])  # 71 blocks: the lanes stride twice
def test_one_window_of_every_block_is_the_meter(lib, m, rows, chs):
    """n = 17640 + 4410 m has no partial block: the window of all NB blocks is mst_loudness_integrated's result, as an fp32 number or
    one ulp from it (the sums are formed in the same order)."""
    rate, n = 44100, 17640 + 4410 * m
    x = torch.from_numpy(R.level_step_noise(rows, chs, n, 60 + m))
    assert WR.num_complete_blocks(n, rate) == m + 1 == lib.mst_loudness_num_blocks(n, rate)
    got, lufs = WR.call_windows(lib, x, rate, tables(lib, rate), m + 1, 1)
    assert tuple(got.shape) == (rows, 1) and torch.isfinite(got).all()
    assert (bits(got[:, 0]) - bits(lufs)).abs().max() <= 1
    assert torch.equal(bits(lufs), bits(torch.from_numpy(meter(lib, x, rate)[0]).float()))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    from mst import _cabi

    def refused(rows, chs, n, rate, W, H):
        return lib.mst_loudness_windows_workspace_bytes(rows, chs, n, rate, W, H) == 0 and WR.count_windows(lib, n, rate, W, H) == 0

    n = 70000
    assert not refused(1, 1, n, 44100, 12, 1) and WR.count_windows(lib, n, 44100, 12, 1) == 1
    assert refused(1, 1, n, 44101, 4, 1)            # the boundary table of 44101 Hz is not equally spaced
    assert refused(1, 1, n, 44100, 0, 1) and refused(1, 1, n, 44100, 4, 0) and refused(1, 1, n, 44100, -1, 1)
    assert refused(1, 1, n, 44100, 13, 1)           # W > NB = 12
    assert refused(1, 1, 17639, 44100, 1, 1)        # shorter than one block
    assert not refused(1, 1, 17640 + 4091 * 4410, 44100, 1, 1)
    assert refused(1, 1, 17640 + 4092 * 4410, 44100, 1, 1)   # more than 4092 blocks
    for rate in (44100, 48000, 22050, 32000, 96000, 88200, 24000):
        assert not refused(1, 1, 4 * rate, rate, 5, 2)
    x = torch.zeros(1, 1, n)
    out = torch.zeros(1, 16)
    with pytest.raises(_cabi.AbiError) as e:
        lib.mst_loudness_windows(x, 1, 1, n, n, n, 44100, tables(lib, 44100), 13, 1, out, None, torch.zeros(8), 0, None)
    assert e.value.code != 0
    with pytest.raises(_cabi.AbiError):  # a workspace one byte short
        nbytes = lib.mst_loudness_windows_workspace_bytes(1, 1, n, 44100, 4, 1)
        lib.mst_loudness_windows(x, 1, 1, n, n, n, 44100, tables(lib, 44100), 4, 1, out, None, torch.zeros(nbytes // 4 + 1), nbytes - 1, None)
