"""The delivery meter's kernels (diff-mst_amd/csrc/mst_truepeak.hip; k_loud_range and k_loud_normalize_limited in mst_loudness.hip)
on the host simulator, against (1) the float64 restatement of their definitions (tests/metering_ref.py - parity with any external
meter is UNPINNED), (2) closed forms: EBU Tech 3341's true-peak sines and Tech 3342's stepped sines, (3) NaN / infinity / silence,
(4) what they refuse and their bit-level properties, (5) the limited normalisation.  The loudness bounds are the meter's own
(tests/test_loudness_hostsim.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import loudness_ref as R
import metering_ref as M
from test_loudness_hostsim import FP32_ALLOWANCE_LU, GATE_MARGIN_LU, lib, meter, tables  # noqa: F401

from mst._cabi import TRUE_PEAK_TILE as TILE


def bits(t):
    return t.contiguous().view(torch.int32)


def cropped(x, front, back):
    """The same values as a last-dimension crop of a longer tensor: rows and channels at odd element offsets, not contiguous."""
    rows, chs, n = x.shape
    full = torch.zeros(rows, chs, front + n + back)
    full[..., front:front + n] = torch.from_numpy(x)
    view = full[..., front:front + n]
    assert not view.is_contiguous() or rows * chs == 1
    return view


def check_true_peak(L, x, F, label, view=None):
    """x numpy (rows, channels, n) fp32; compares the kernels with the restatement item by item and channel by channel."""
    h = M.lib_taps(L, F)
    t = torch.from_numpy(x) if view is None else view
    peak, chan = M.call_true_peak(L, t, F)
    worst = 0.0
    for r in range(x.shape[0]):
        xmax = float(np.max(np.abs(x[r])))
        bound = M.true_peak_bound(h, F, xmax)
        per = [M.true_peak(x[r, c:c + 1], h, F) for c in range(x.shape[1])]
        err = max(abs(float(chan[r, c]) - per[c]) for c in range(x.shape[1]))
        err = max(err, abs(float(peak[r]) - max(per)))
        worst = max(worst, err / xmax if xmax else err)
        assert err <= bound, f"{label} row {r}: |TP - TP_f64| = {err:.3e} > {bound:.3e}"
        assert float(peak[r]) == float(chan[r].max()) and float(peak[r]) >= xmax  # the sample peak is contained
    print(f"\n[{label}] worst |TP - TP_f64| / max|x| = {worst:.3e} (bound {M.true_peak_bound(h, F, 1.0):.3e})")
    return peak, chan


# ---- 1. true peak against the restatement ---------------------------------------------------------------------------------------
LENGTHS = [1, 5, TILE - 1, TILE, TILE + 1, TILE + 13, 2 * TILE + 7]
SHAPES = [(1, 1), (3, 2), (1, 5), (3, 1), (1, 2), (3, 5), (3, 2)]  # (rows, channels) of the length at the same place


@pytest.mark.parametrize("F", [4, 2])
@pytest.mark.parametrize("n,shape", list(zip(LENGTHS, SHAPES)))
def test_true_peak_matches_the_float64_restatement(lib, n, shape, F):
    rows, chs = shape
    rng = np.random.default_rng(100 * F + n)
    x = (0.3 * rng.standard_normal((rows, chs, n)) * (10.0 ** (-0.35 * np.arange(rows)))[:, None, None]).astype(np.float32)
    check_true_peak(lib, x, F, f"F={F} {rows}x{chs}x{n}")


@pytest.mark.parametrize("F", [4, 2])
def test_true_peak_reads_a_strided_view_in_place(lib, F):
    rng = np.random.default_rng(7 + F)
    x = (0.3 * rng.standard_normal((3, 2, TILE + 13))).astype(np.float32)
    view = cropped(x, 3, 5)
    assert view.stride(0) % 2 == 0 and (view.storage_offset() % 4, view.stride(1) % 4) == (3, 1)  # rows on every 4-byte alignment
    a, ac = check_true_peak(lib, x, F, f"F={F} strided", view=view)
    b, bc = M.call_true_peak(lib, torch.from_numpy(x), F)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(ac), bits(bc))


def placed(kind, F):
    """One channel of 2 TILE + 7 samples of low-level noise with a few large samples placed so that the maximum of the interpolated
    signal falls where `kind` says -> (x (1, 1, n) fp32, predicate on the restatement's arg-max k)."""
    n = 2 * TILE + 7
    x = 0.01 * np.random.default_rng(5).standard_normal(n)
    if kind == "tile boundary":  # between the last sample of the first tile and the first of the second
        x[TILE - 1] = x[TILE] = 0.7
        ok = lambda k: F * (TILE - 1) + 24 < k < F * TILE + 24
    elif kind == "halo":  # both large samples lie in front of the second tile, the maximum is the second tile's first position
        x[TILE - 6] = x[TILE - 5] = 0.7
        ok = lambda k: k // F == TILE and k % F != 0
        assert F == 4  # at F = 4 the centre tap sits 6 positions behind its sample
    else:  # "tail": after the last sample; the signal ends on a large step
        x[n - 32:] = 0.7 * (np.arange(32) + 1.0) / 32.0 * (-1.0) ** (np.arange(32) + 1)  # an alternating ramp, cut off at its top
        ok = lambda k: k > F * (n - 1) + 24
    return x.astype(np.float32).reshape(1, 1, n), ok


@pytest.mark.parametrize("kind,F", [("tile boundary", 4), ("tile boundary", 2), ("halo", 4), ("tail", 4), ("tail", 2)])
def test_true_peak_maximum_in_every_region(lib, kind, F):
    x, ok = placed(kind, F)
    h = M.lib_taps(lib, F)
    tp, (_, k) = M.true_peak(x[0], h, F, return_argmax=True)
    assert ok(k), f"{kind}: the restatement's maximum sits at k = {k}"  # before the kernel is looked at
    assert tp > 1.05 * float(np.max(np.abs(x)))  # and it is an inter-sample peak
    check_true_peak(lib, x, F, f"F={F} maximum at the {kind}")


# ---- 2. coefficients and closed forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [4, 2])
def test_coefficients_are_the_closed_form(lib, F):
    h = M.lib_taps(lib, F)
    ref = M.closed_form_taps(F)
    ident = np.arange(M.TAPS) % F == 0
    # phase 0 is exactly the identity: where the closed form holds sin(pi k) it holds rounding noise of pi, far below any tap
    assert h[24] == 1.0 and not h[ident & (np.arange(M.TAPS) != 24)].any()
    assert np.max(np.abs(ref[ident & (np.arange(M.TAPS) != 24)])) < 2.0 ** -50
    want = ref[~ident].astype(np.float32)
    ulps = np.abs(h[~ident].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1 and h[~ident].all()  # libm may differ from numpy in the last float64 bit
    sums = [float(np.abs(h[p::F].astype(np.float64)).sum()) for p in range(F)]
    print(f"\n[F={F}] sum |h| per phase: {[round(s, 4) for s in sums]}, worst {ulps.max()} ulp from the closed form")
    if F == 4:
        assert [round(s, 3) for s in sums] == [1.0, 1.631, 1.864, 1.631]


SINES = [(0.5, 4, 0.0), (0.5, 4, 45.0), (0.5, 6, 60.0), (0.5, 8, 67.5), (1.41, 4, 45.0)]  # amplitude, fs / f, phase in degrees


@pytest.mark.parametrize("amp,div,phase", SINES)
def test_true_peak_of_sines_reads_their_amplitude(lib, amp, div, phase):
    """EBU Tech 3341's true-peak cases, read within its +0.2 / -0.4 dB.  20 ms raised-cosine fades: an abrupt start overshoots by up
    to 0.65 dB, which is the band-limited truth of a truncated sine and no meter error."""
    rate, n = 48000, 4800
    i = np.arange(n)
    fade = np.ones(n)
    nf = rate // 50
    fade[:nf] = 0.5 * (1.0 - np.cos(math.pi * i[:nf] / nf))
    fade[-nf:] = fade[:nf][::-1]
    x = (amp * np.sin(2.0 * math.pi * i / div + math.radians(phase)) * fade).astype(np.float32).reshape(1, 1, n)
    want = 20.0 * math.log10(amp)
    ref = float(M.dbtp(M.true_peak(x[0], M.lib_taps(lib, 4), 4)))
    got = float(M.dbtp(float(M.call_true_peak(lib, torch.from_numpy(x), 4)[0][0])))
    sample = 20.0 * math.log10(float(np.max(np.abs(x))))
    print(f"\n[sine fs/{div} {phase} deg] {want:.3f} dB: restatement {ref - want:+.4f}, kernel {got - want:+.4f}, sample peak {sample - want:+.3f}")
    assert -0.4 <= ref - want <= 0.2
    assert -0.4 <= got - want <= 0.2
    if (div, phase) == (4, 45.0):
        assert sample - want < -3.0  # what a sample-peak meter misses


def test_nan_infinity_and_silence(lib):
    rng = np.random.default_rng(3)
    x = (0.2 * rng.standard_normal((4, 2, TILE + 13))).astype(np.float32)
    x[3] = 0.0
    clean, clean_c = M.call_true_peak(lib, torch.from_numpy(x), 4)
    y = x.copy()
    y[1, 1, TILE + 2] = np.nan
    y[2, 0, 17] = np.inf
    got, got_c = M.call_true_peak(lib, torch.from_numpy(y), 4)
    assert torch.isnan(got[1]) and torch.isnan(got_c[1, 1]) and torch.equal(bits(got_c[1, 0]), bits(clean_c[1, 0]))
    assert got[2] == float("inf") and got_c[2, 0] == float("inf") and torch.equal(bits(got_c[2, 1]), bits(clean_c[2, 1]))
    assert torch.equal(bits(got[0]), bits(clean[0])) and torch.equal(bits(got[3]), bits(clean[3]))
    assert float(got[3]) == 0.0 and np.isneginf(M.dbtp(float(got[3])))
    assert math.isnan(M.true_peak(y[1], M.lib_taps(lib, 4), 4))


def test_sample_peak_comes_from_the_same_pass(lib):
    rng = np.random.default_rng(4)
    x = (0.2 * rng.standard_normal((4, 2, TILE + 13))).astype(np.float32)
    x[1, 0, 5] = np.nan
    x[2, 1, TILE + 12] = -np.inf
    x[3] = 0.0
    t = cropped(x, 3, 2)
    nbytes = lib.mst_true_peak_workspace_bytes(4, 2, x.shape[2], 4)
    ws = torch.full((nbytes // 4 + 1,), float("nan"))
    (pb, peak), (sb, sample) = M.guarded((4,), "cpu"), M.guarded((4,), "cpu")
    lib.mst_true_peak_sample(t, 4, 2, x.shape[2], t.stride(0), t.stride(1), 4, peak, None, sample, ws, nbytes, None)
    assert M.guards_intact(pb) and M.guards_intact(sb)
    assert float(sample[0]) == float(np.max(np.abs(x[0]))) and float(sample[3]) == 0.0  # a maximum is exact
    assert torch.isnan(sample[1]) and torch.isnan(peak[1]) and sample[2] == float("inf") and peak[2] == float("inf")
    assert torch.equal(bits(peak), bits(M.call_true_peak(lib, t, 4, per_channel=False)[0])) and float(peak[0]) >= float(sample[0])


# ---- 3. short-term loudness and range against the restatement -------------------------------------------------------------------
def check_range(L, x, rate, H, label, view=None, expect_losses=False):
    rows = x.shape[0]
    ref = []
    lost_abs = lost_rel = False
    for r in range(rows):  # the restatement alone first: no window may sit on a gate
        E, l = M.short_term(x[r], rate, H)
        lra, l_lo, l_hi, a, f = M.loudness_range(E)
        m_rel, m_abs = M.range_margins(l)
        assert m_rel > GATE_MARGIN_LU and m_abs > GATE_MARGIN_LU, f"{label} row {r}: a window sits on a gate, change the seed"
        lost_abs |= len(a) < len(E)
        lost_rel |= len(f) < len(a)
        ref.append((E, l, lra, l_lo, l_hi, a, f))
    if expect_losses:
        assert lost_abs and lost_rel
    t = torch.from_numpy(x) if view is None else view
    out = M.call_range(L, t, rate, tables(L, rate), H)
    assert M.count_short_term(L, x.shape[2], rate, H) == M.num_short_term(x.shape[2], rate, H) == out["short"].shape[1]
    worst_l = worst_r = 0.0
    for r in range(rows):
        E, l, lra, l_lo, l_hi, a, f = ref[r]
        got = out["short"][r].double().numpy()
        fin = np.isfinite(l)
        assert np.array_equal(np.isfinite(got), fin) and np.all(np.isneginf(got[~fin]))
        above = l > -70.0
        if above.any():
            worst_l = max(worst_l, float(np.max(np.abs(got - l)[above])))
        ga, _, gf = M.range_gates(got)
        assert (ga, gf) == (a, f), f"{label} row {r}: gate sets differ"
        worst_r = max(worst_r, abs(float(out["range"][r]) - lra))
        if f:
            worst_r = max(worst_r, abs(float(out["bounds"][r, 0]) - l_lo), abs(float(out["bounds"][r, 1]) - l_hi))
        else:
            assert float(out["range"][r]) == 0.0 and torch.isnan(out["bounds"][r]).all()
    print(f"\n[{label}] |l_k - l_k_f64| = {worst_l:.3e} LU, |LRA - LRA_f64| = {worst_r:.3e} LU (bound {FP32_ALLOWANCE_LU:.1e})")
    assert worst_l <= FP32_ALLOWANCE_LU and worst_r <= FP32_ALLOWANCE_LU
    lufs, blocks = meter(L, t, rate)  # mst_loudness_integrated
    assert np.array_equal(out["lufs"].double().numpy(), lufs) and np.array_equal(out["blocks"].double().numpy(), blocks)
    return out


RANGE_CASES = [(rate, H, nseg) for rate in (44100, 48000) for H in (1, 10) for nseg in (30, 31, 57)]


@pytest.mark.parametrize("rate,H,nseg", RANGE_CASES)
def test_short_term_and_range_match_the_float64_restatement(lib, rate, H, nseg):
    n = nseg * (rate // 10) + 17
    rows, chs = (2, 2) if nseg == 31 else (1, 1)
    x = R.level_step_noise(rows, chs, n, 200 + nseg + H)
    view = cropped(x, 3, 6) if nseg == 31 else None
    check_range(lib, x, rate, H, f"{rate} Hz H={H} NSEG={nseg}", view=view)


def test_range_gates_remove_windows(lib):
    """12 s: the 30 dB and the 1e-6 stretch of level_step_noise are 4.2 s each, so a 3 s window fits into either - the restatement
    shows a window lost to the absolute gate and one lost to the relative gate."""
    rate = 44100
    x = R.level_step_noise(1, 2, 120 * 4410 + 5, 77)
    out = check_range(lib, x, rate, 10, "44100 Hz H=10 NSEG=120", expect_losses=True)
    assert float(out["range"][0]) > 0.0


@pytest.mark.parametrize("lo_db,hi_db,want", [(-20.0, -30.0, 10.0), (-20.0, -15.0, 5.0), (-40.0, -20.0, 20.0)])
def test_range_of_stepped_sines(lib, lo_db, hi_db, want):
    """EBU Tech 3342's stepped 1 kHz sines, 10 s + 10 s (eight one-second hops wholly inside each level), +- 1 LU."""
    rate = 22050
    i = np.arange(10 * rate)
    s = np.sin(2.0 * math.pi * 1000.0 * i / rate)
    x = np.concatenate([10.0 ** (lo_db / 20.0) * s, 10.0 ** (hi_db / 20.0) * s]).astype(np.float32).reshape(1, 1, -1)
    E, _ = M.short_term(x[0], rate, 10)
    ref = M.loudness_range(E)[0]
    assert abs(ref - want) <= 1.0
    out = M.call_range(lib, torch.from_numpy(x), rate, tables(lib, rate), 10, want=())
    got = float(out["range"][0])
    print(f"\n[stepped sine {lo_db} / {hi_db} dBFS] restatement {ref:.4f} LU, kernel {got:.4f} LU")
    assert abs(got - want) <= 1.0 and abs(got - ref) <= FP32_ALLOWANCE_LU


# ---- 4. refusals and bit-level properties ---------------------------------------------------------------------------------------
def test_refusals(lib):
    from mst import _cabi

    L = lib
    assert [M.lib_factor(L, r) for r in (22050, 44100, 48000, 95999, 96000, 191999, 192000, 384000, 0, -1)] == [4, 4, 4, 4, 2, 2, 0, 0, 0, 0]
    with pytest.raises(_cabi.AbiError):
        L.mst_true_peak_factor(44100, None)
    with pytest.raises(_cabi.AbiError):
        L.mst_true_peak_coefficients(3, (ctypes.c_float * 49)())
    with pytest.raises(_cabi.AbiError):
        L.mst_true_peak_coefficients(4, None)
    assert L.mst_true_peak_workspace_bytes(1, 1, 1, 4) > 0 and L.mst_true_peak_workspace_bytes(1, 1, 1, 2) > 0
    for bad in ((1, 1, 0, 4), (0, 1, 10, 4), (1, 0, 10, 4), (1, 1, 10, 3), (1, 1, 10, 0), (65536, 1, 10, 4), (13108, 5, 10, 4)):
        assert L.mst_true_peak_workspace_bytes(*bad) == 0
    x, out, ws = torch.zeros(1, 1, 100), torch.zeros(1), torch.zeros(64)
    nbytes = L.mst_true_peak_workspace_bytes(1, 1, 100, 4)
    for args in ((None, 1, 1, 100, 100, 100, 4, out, None, ws, nbytes), (x, 1, 1, 100, 100, 100, 4, None, None, ws, nbytes),
                 (x, 1, 1, 100, 100, 100, 4, out, None, None, nbytes), (x, 1, 1, 100, 100, 100, 4, out, None, ws, nbytes - 1),
                 (x, 1, 1, 100, 100, 100, 8, out, None, ws, nbytes), (x, 1, 1, 100, -1, 100, 4, out, None, ws, nbytes)):
        with pytest.raises(_cabi.AbiError) as e:
            L.mst_true_peak(*args, None)
        assert e.value.code != 0

    def refused(rows, chs, n, rate, H):
        return L.mst_loudness_range_workspace_bytes(rows, chs, n, rate, H) == 0 and M.count_short_term(L, n, rate, H) == 0

    n = 30 * 4410
    assert not refused(1, 1, n, 44100, 10) and M.count_short_term(L, n, 44100, 10) == 1
    assert refused(1, 1, n - 1, 44100, 10)                                   # shorter than 3 s
    assert refused(1, 1, n, 44100, 0) and refused(1, 1, n, 44100, 31) and not refused(1, 1, n, 44100, 30)
    assert refused(1, 1, 4 * 44101, 44101, 10)                               # unequal table
    assert L.mst_loudness_range_workspace_bytes(1, 6, n, 44100, 10) == 0 and refused(1, 1, n, 8000, 10)
    with pytest.raises(_cabi.AbiError):
        L.mst_loudness_num_short_term(n, 44100, 10, None)
    x = torch.zeros(1, 1, n)
    t = tables(L, 44100)
    nbytes = L.mst_loudness_range_workspace_bytes(1, 1, n, 44100, 10)
    ws = torch.zeros(nbytes // 4 + 1)
    lra = torch.zeros(1)
    for args in ((None, 1, 1, n, n, n, 44100, t, 10, None, lra, None, None, None, ws, nbytes),
                 (x, 1, 1, n, n, n, 44100, None, 10, None, lra, None, None, None, ws, nbytes),
                 (x, 1, 1, n, n, n, 44100, t, 10, None, None, None, None, None, ws, nbytes),
                 (x, 1, 1, n, n, n, 44100, t, 10, None, lra, None, None, None, None, nbytes),
                 (x, 1, 1, n, n, n, 44100, t, 10, None, lra, None, None, None, ws, nbytes - 1),
                 (x, 1, 1, n, n, n, 44100, t, 31, None, lra, None, None, None, ws, nbytes)):
        with pytest.raises(_cabi.AbiError):
            L.mst_loudness_range(*args, None)
    y, l1, g = torch.zeros(1, 1, n), torch.zeros(1), torch.zeros(1)
    for args in ((None, y, l1, l1, 1, 1, n, n, n, -14.0, -70.0, -1.0, g, None), (x, y, l1, None, 1, 1, n, n, n, -14.0, -70.0, -1.0, g, None),
                 (x, y, l1, l1, 1, 1, n, n, n, -14.0, -70.0, -1.0, None, None), (x, y, l1, l1, 1, 1, n, n, n, -14.0, -70.0, float("nan"), g, None)):
        with pytest.raises(_cabi.AbiError):
            L.mst_loudness_normalize_limited(*args, None)


def test_two_calls_and_any_workspace_are_bit_identical(lib):
    rate, n = 44100, 31 * 4410 + 9
    x = torch.from_numpy(R.level_step_noise(2, 2, n, 91))
    t = tables(lib, rate)
    a, b, z = (M.call_range(lib, x, rate, t, 1, fill=f) for f in (float("nan"), float("nan"), 0.0))
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])) and torch.equal(bits(a[k]), bits(z[k])), k
    hop = M.call_range(lib, x, rate, t, 1, want=())  # every optional output NULL
    assert torch.equal(bits(hop["range"]), bits(a["range"]))
    p, pc = M.call_true_peak(lib, x, 4)
    q, qc = M.call_true_peak(lib, x, 4, fill=0.0)
    r, _ = M.call_true_peak(lib, x, 4, per_channel=False)
    assert torch.equal(bits(p), bits(q)) and torch.equal(bits(pc), bits(qc)) and torch.equal(bits(p), bits(r))


# ---- 5. the limited normalisation -----------------------------------------------------------------------------------------------
def test_normalize_limited(lib):
    L, rate, n, target, ceiling = lib, 44100, 20001, -23.0, -1.0
    rng = np.random.default_rng(8)
    x = np.zeros((3, 2, n), dtype=np.float32)
    x[0] = 0.001 * rng.standard_normal((2, n))
    x[0, 1, 9000:9002] = 0.5                       # sparse: quiet, with a peak the loudness gain would push over full scale
    x[1] = 0.1 * rng.standard_normal((2, n))       # dense: reaches the target below the ceiling
    view = cropped(x, 1, 4)
    lufs = torch.from_numpy(meter(L, view, rate)[0]).float()
    tp, _ = M.call_true_peak(L, view, 4)
    yb, y = M.guarded((3, 2, n), "cpu")
    gb, gain = M.guarded((3,), "cpu")
    keep = torch.full((3,), 7, dtype=torch.uint8)
    L.mst_loudness_normalize_limited(view, y, lufs, tp, 3, 2, n, view.stride(0), view.stride(1), target, float("-inf"), ceiling, gain,
                                     keep, None)
    assert M.guards_intact(yb) and M.guards_intact(gb)
    plain, pkeep = torch.full((3, 2, n), float("nan")), torch.zeros(3, dtype=torch.uint8)
    L.mst_loudness_normalize(view, plain, lufs, 3, 2, n, view.stride(0), view.stride(1), target, float("-inf"), pkeep, None)
    assert keep.tolist() == pkeep.tolist() == [1, 1, 0] and not y[2].any() and torch.equal(bits(y[2]), bits(plain[2]))
    assert gain[2] == float("-inf")
    l64, tp64 = lufs.double().numpy(), tp.double().numpy()
    assert target - l64[0] > ceiling - 20.0 * math.log10(tp64[0]) and target - l64[1] < ceiling - 20.0 * math.log10(tp64[1])
    # the gain is one fp32 rounding of a float64 expression of the kernel's own inputs (the device's log10 may differ in the last place)
    assert abs(float(gain[0]) - (ceiling - 20.0 * math.log10(tp64[0]))) <= 2.0 ** -22 * abs(float(gain[0]))
    assert abs(float(gain[1]) - (target - l64[1])) <= 2.0 ** -22 * abs(float(gain[1]))
    assert torch.equal(bits(y[1]), bits(plain[1]))  # below the ceiling: mst_loudness_normalize's arithmetic
    g0 = 10.0 ** (ceiling / 20.0) / tp64[0]
    assert np.allclose(y[0].double().numpy(), x[0].astype(np.float64) * np.float32(g0).astype(np.float64), rtol=2.0 ** -22, atol=0.0)
    # re-measured: the gain (one rounding, and the pow / division's last place) and every product (one rounding, carried through the
    # interpolator: at most 2^-24 sum |h| max |y|) round, and the meter itself is within its bound
    again, _ = M.call_true_peak(L, y, 4)
    h = M.lib_taps(L, 4)
    lin = 10.0 ** (ceiling / 20.0)
    for r in (0, 1):
        ymax = float(y[r].abs().max())
        slack = lin * 2.0 ** -22 + (2.0 ** -24 * M.sum_abs_taps(h, 4) * ymax) + M.true_peak_bound(h, 4, ymax)
        print(f"\n[limited row {r}] gain {float(gain[r]):+.4f} dB, true peak after {float(M.dbtp(float(again[r]))):+.5f} dBTP (ceiling {ceiling})")
        assert float(again[r]) <= lin + slack
    assert abs(float(again[0]) - lin) <= lin * 1e-5  # the capped row sits AT the ceiling
