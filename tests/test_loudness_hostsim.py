"""The loudness-meter kernels (diff-mst_amd/csrc/mst_loudness.hip) on the host simulator, against
(1) the closed-form level of stationary sines and the BS.1770 calibration point, (2) the float64 restatement of
pyloudnorm's algorithm (tests/loudness_ref.py - parity with the package itself is UNPINNED, it is not installed),
(3) edge cases, (4) the normalisation kernel, (5) the host-side block-boundary table."""
import math

import numpy as np
import pytest
import torch

import loudness_ref as R

# |L_hip - L_f64| allowed, derived: the loudness feeds a linear gain 10^(d/20), so e LU are a relative gain error of
# e ln(10)/20 = 0.115 e; run_diffmst's mix is tested to 1e-4 relative and the meter gets a tenth of that: 1e-5 / 0.115
FP32_ALLOWANCE_LU = 8.7e-5
GATE_MARGIN_LU = 1e-3  # ten times the bound (rounded up): no block of a test input may sit closer to a gate
# float64 restatement vs the closed form a^2/2 |H|^2 of a stationary sine, 10 s: the start-up transient of the 38 Hz high pass in
# the first blocks and the non-integer number of periods per block.  Measured: 2.888e-4 LU (100 Hz), 6.0e-6 (997 Hz), 2.5e-6 (4 kHz)
# at 44100 Hz, 5.9e-6 (997 Hz at 48000 Hz)
RESTATEMENT_VS_CLOSED_FORM_LU = 2.9e-4
CLOSED_FORM_TOL_LU = RESTATEMENT_VS_CLOSED_FORM_LU + FP32_ALLOWANCE_LU


@pytest.fixture(scope="module")
def lib():
    from hostsim import harness

    return harness.lib()


_TABLES = {}


def tables(L, rate):
    if rate not in _TABLES:
        nbytes = L.mst_loudness_tables_bytes(rate)
        assert nbytes > 0
        t = torch.zeros(nbytes // 4, dtype=torch.int32)
        L.mst_loudness_init_tables(rate, t, None)
        _TABLES[rate] = t
    return _TABLES[rate]


def meter(L, x, rate):
    """x: float32 tensor (rows, channels, n), any row / channel stride -> (lufs (rows,), block loudness (rows, nb)) float64 numpy."""
    rows, chs, n = x.shape
    assert x.stride(2) == 1
    nbytes = L.mst_loudness_workspace_bytes(rows, chs, n, rate)
    nb = L.mst_loudness_num_blocks(n, rate)
    assert nbytes > 0 and nb == R.num_blocks(n, rate)
    ws = torch.full((nbytes // 8 + 1,), float("nan"), dtype=torch.float64)  # the kernels must not rely on a cleared workspace
    lufs = torch.full((rows,), float("nan"))
    blocks = torch.full((rows, nb), float("nan"))
    L.mst_loudness_integrated(x, rows, chs, n, x.stride(0), x.stride(1), rate, tables(L, rate), lufs, blocks, ws, nbytes, None)
    return lufs.double().numpy(), blocks.double().numpy()


def reference(x, rate):
    out = [R.integrated_loudness(x[r].T.astype(np.float64), rate, return_blocks=True) for r in range(x.shape[0])]
    return np.array([o[0] for o in out]), np.stack([o[1] for o in out])


def check_against_restatement(lufs, blocks, ref_lufs, ref_blocks, label):
    """Margin pre-check on the restatement alone, then value and gate-set comparison.  Returns the measured errors."""
    for r in range(len(ref_lufs)):
        m_rel, m_abs = R.gate_margins(ref_blocks[r])
        assert m_rel > GATE_MARGIN_LU and m_abs > GATE_MARGIN_LU, f"{label} row {r}: a block sits on a gate, change the seed"
    err_l = float(np.max(np.abs(lufs - ref_lufs)))
    above = ref_blocks > R.ABS_GATE
    err_b = float(np.max(np.abs(blocks - ref_blocks)[above]))
    print(f"\n[{label}] |L - L_f64| = {err_l:.3e} LU, per block = {err_b:.3e} LU (bound {FP32_ALLOWANCE_LU:.1e})")
    assert err_l <= FP32_ALLOWANCE_LU and err_b <= FP32_ALLOWANCE_LU
    for r in range(len(ref_lufs)):
        a, _, f = R.gate_sets(blocks[r])
        ra, _, rf = R.gate_sets(ref_blocks[r])
        assert a == ra and f == rf, f"{label} row {r}: gate sets differ"
        assert 0 < len(rf) < len(ra) < len(ref_blocks[r]) or len(ref_blocks[r]) == 1  # both gates remove something
    return err_l, err_b


# ---- 1. closed form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,freq,amp", [(44100, 100.0, 0.5), (44100, 997.0, 1.0), (44100, 4000.0, 0.25), (48000, 997.0, 1.0)])
def test_stationary_sine_matches_the_closed_form(lib, rate, freq, amp):
    n = 10 * rate
    x = amp * np.sin(2.0 * math.pi * freq * np.arange(n) / rate)
    closed = -0.691 + 10.0 * math.log10(amp * amp / 2.0 * R.response_sq(rate, freq))
    ref = R.integrated_loudness(x, rate)
    got = meter(lib, torch.from_numpy(x.astype(np.float32)).view(1, 1, n), rate)[0][0]
    print(f"\n[sine {freq} Hz @ {rate}] closed form {closed:.6f}, restatement {ref:.6f} ({ref - closed:+.3e}), kernel {got:.6f} ({got - closed:+.3e})")
    assert abs(ref - closed) <= RESTATEMENT_VS_CLOSED_FORM_LU
    assert abs(got - closed) <= CLOSED_FORM_TOL_LU
    if freq == 997.0 and amp == 1.0:
        # the standard's calibration point: 997 Hz, 0 dBFS, one channel -> -3.01 LKFS, at the +-0.1 LU of its conformance material
        assert abs(ref - (-3.01)) <= 0.1 and abs(got - (-3.01)) <= 0.1


# ---- 2. against the restatement -----------------------------------------------------------------------------------------------
CASES = [
    # rate, rows, channels, n, (front pad, back pad) of the longer tensor the rows are cropped from, seed
    (44100, 1, 1, 262144, (0, 0), 11),
    (44100, 3, 2, 70000, (8, 120), 12),      # aligned crop: 16-byte loads on strided rows
    (48000, 2, 1, 70001, (3, 2), 13),        # n % 4 != 0 and rows that are not 16-byte aligned
    (44100, 1, 5, 17640, (0, 0), 14),        # exactly one block, all five channel weights
    (48000, 1, 5, 70000, (0, 0), 15),
    (44100, 2, 2, 17641, (0, 0), 16),
]


@pytest.mark.parametrize("rate,rows,chs,n,pad,seed", CASES)
def test_meter_matches_the_float64_restatement(lib, rate, rows, chs, n, pad, seed):
    x = R.level_step_noise(rows, chs, n, seed)
    ref_lufs, ref_blocks = reference(x, rate)
    full = torch.zeros(rows, chs, pad[0] + n + pad[1])
    full[..., pad[0]:pad[0] + n] = torch.from_numpy(x)
    view = full[..., pad[0]:pad[0] + n]
    assert pad == (0, 0) or not view.is_contiguous()
    lufs, blocks = meter(lib, view, rate)
    check_against_restatement(lufs, blocks, ref_lufs, ref_blocks, f"{rate} Hz {rows}x{chs}x{n}")


# ---- 3. edge cases ------------------------------------------------------------------------------------------------------------
def test_silent_and_sub_gate_rows(lib):
    n, rate = 30000, 44100
    x = torch.from_numpy(R.level_step_noise(4, 1, n, 21))
    x[1] = 0.0            # silence
    x[2] *= 1e-5          # every block far below the absolute gate
    lufs, blocks = meter(lib, x, rate)
    assert np.isneginf(lufs[1]) and np.all(np.isneginf(blocks[1]))
    assert np.isneginf(lufs[2]) and np.all(blocks[2] < R.ABS_GATE) and np.all(np.isfinite(blocks[2]))
    assert np.isfinite(lufs[0]) and np.isfinite(lufs[3]) and not np.any(np.isnan(blocks))
    ref = R.integrated_loudness(x[2].T.double().numpy(), rate)
    assert np.isneginf(ref)
    # normalisation: the silent and the sub-floor row are dropped and written as zeros
    y = torch.full((4, 1, n), float("nan"))
    keep = torch.full((4,), 7, dtype=torch.uint8)
    lt = torch.from_numpy(lufs).float()
    lib.mst_loudness_normalize(x, y, lt, 4, 1, n, x.stride(0), x.stride(1), -48.0, -80.0, keep, None)
    assert keep.tolist() == [1, 0, 0, 1]
    assert torch.isfinite(y).all() and not y[1].any() and not y[2].any() and y[0].any() and y[3].any()


def test_short_signals_are_refused(lib):
    import mst.utils as U
    from mst import _cabi

    assert lib.mst_loudness_workspace_bytes(1, 1, 17639, 44100) == 0 and lib.mst_loudness_num_blocks(17639, 44100) == 0
    assert lib.mst_loudness_workspace_bytes(1, 1, 17640, 44100) > 0 and lib.mst_loudness_num_blocks(17640, 44100) == 1
    assert lib.mst_loudness_workspace_bytes(1, 6, 70000, 44100) == 0      # five channels at most
    assert lib.mst_loudness_workspace_bytes(1, 1, 70000, 8000) == 0       # unsupported rate
    with pytest.raises(_cabi.AbiError) as e:
        lib.mst_loudness_integrated(None, 1, 1, 70000, 70000, 70000, 44100, None, None, None, None, 0, None)
    assert e.value.code != 0
    with pytest.raises(_cabi.AbiError) as e:
        lib.mst_loudness_normalize(None, None, None, 1, 1, 70000, 70000, 70000, -48.0, -80.0, None, None)
    assert e.value.code != 0
    with pytest.raises(ValueError, match="Audio must have length greater than the block size."):
        U.integrated_loudness(torch.zeros(1, 17639))
    with pytest.raises(ValueError, match="Audio must have length greater than the block size."):
        U.LoudnessMeter(44100).integrated_loudness(np.zeros(17639))
    with pytest.raises(ValueError, match="five channels"):
        U.integrated_loudness(torch.zeros(6, 20000))


@pytest.mark.parametrize("rows", [1, 33])
def test_two_calls_are_bit_identical(lib, rows):
    x = torch.from_numpy(R.level_step_noise(rows, 1, 17640 + 4410, 30 + rows))
    a, ab = meter(lib, x, 44100)
    b, bb = meter(lib, x, 44100)
    assert np.array_equal(a, b) and np.array_equal(ab, bb) and np.all(np.isfinite(a))
    ref, _ = reference(x.numpy()[:: max(1, rows // 3)], 44100)
    assert np.max(np.abs(a[:: max(1, rows // 3)] - ref)) <= FP32_ALLOWANCE_LU


# ---- 4. normalisation ---------------------------------------------------------------------------------------------------------
def test_normalize_gains(lib):
    n, rate, target = 20001, 44100, -23.0
    full = torch.zeros(3, 2, n + 5)
    full[..., 1:n + 1] = torch.from_numpy(R.level_step_noise(3, 2, n, 41))
    x = full[..., 1:n + 1]
    lufs, _ = meter(lib, x, rate)
    lt = torch.from_numpy(lufs).float()
    y = torch.full((3, 2, n), float("nan"))
    keep = torch.zeros(3, dtype=torch.uint8)
    lib.mst_loudness_normalize(x, y, lt, 3, 2, n, x.stride(0), x.stride(1), target, float("-inf"), keep, None)
    assert keep.tolist() == [1, 1, 1]
    gain = 10.0 ** ((target - lt.double().numpy()) / 20.0)  # float64, from the kernel's own L
    want = x.double().numpy() * gain.astype(np.float32).astype(np.float64)[:, None, None]
    # one fp32 rounding of the gain (the device's pow may differ from numpy's in the last place) and one of the product
    assert np.allclose(y.double().numpy(), want, rtol=2.0 ** -22, atol=0.0)
    # and the normalised signal measures at the target
    again, _ = meter(lib, y, rate)
    assert np.max(np.abs(again - target)) < 1e-4


# ---- 5. host logic: the block-boundary table ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [44100, 48000, 22050])
def test_boundary_table_is_pyloudnorms_expression(lib, rate):
    bounds = tables(lib, rate)[:4096].numpy()  # the table opens with 4096 int32 boundaries (include/diffmst_hip.h)
    off_grid_ref, off_grid_tab = [], []
    for j in range(1000):
        lo, hi = R.block_bounds(j, rate)
        assert (int(bounds[j]), int(bounds[j + 4])) == (lo, hi)
        if lo != (j * rate) // 10:
            off_grid_ref.append(j)
        if int(bounds[j]) != (j * rate) // 10:
            off_grid_tab.append(j)
    print(f"\n[{rate} Hz] boundaries that differ from j * rate / 10: {len(off_grid_ref)} of 1000")
    assert off_grid_tab == off_grid_ref
