"""Float64 restatement of the three definitions of include/diffmst_hip.h's delivery meter: true peak (BS.1770-4 Annex 2
with libebur128's 49-tap Hann-windowed sinc, as a FULL convolution), short-term loudness (3 s windows over the song K-weighted once)
and loudness range (EBU Tech 3342).  Also the calls through a bound library that the simulator and the GPU tests share.

PARITY UNPINNED: no external meter is installed where this project is built and tested.  What ties the restatement to the standards
are the closed-form cases asserted in tests/test_metering_hostsim.py (Tech 3341's true-peak sines, Tech 3342's stepped sines).

The fp32 taps come from ``mst_true_peak_coefficients`` (the test of the coefficients compares them with ``closed_form_taps``); the
K-weighting and the boundaries come from loudness_ref.py.  No arithmetic here is done by the code under test.

TEST INFRASTRUCTURE: numpy only (and torch / ctypes for the calls).
"""
import ctypes
import math

import numpy as np
import torch

import loudness_ref as R

TAPS = 49
SHORT_SEGMENTS = 30  # a short-term window: 30 segments of rate / 10 samples


def factor_of(rate):
    return 4 if rate < 96000 else 2 if rate < 192000 else 0


def closed_form_taps(F):
    """h[j] = sinc((j - 24) / F) * 0.5 * (1 - cos(2 pi j / 48)) in numpy float64, as written (sin(pi k) is not exactly 0 here)."""
    j = np.arange(TAPS, dtype=np.float64)
    t = (j - 24.0) / F
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    return s * 0.5 * (1.0 - np.cos(2.0 * np.pi * j / 48.0))


def interpolate(x, h, F):
    """x (n,) -> y (F (n - 1) + 49,) float64: the zero-stuffed signal convolved with the taps, every output kept."""
    x = np.asarray(x, dtype=np.float64)
    up = np.zeros(F * (len(x) - 1) + 1)
    up[::F] = x
    with np.errstate(invalid="ignore"):
        return np.convolve(up, np.asarray(h, dtype=np.float64))


def true_peak(x, h, F, return_argmax=False):
    """x (channels, n) -> linear true peak (float64; NaN when a sample is NaN), optionally (channel, k) of the maximum."""
    best, where = 0.0, (0, 0)
    for c in range(x.shape[0]):
        y = np.abs(interpolate(x[c], h, F))
        if np.isnan(y).any():
            return (float("nan"), None) if return_argmax else float("nan")
        k = int(np.argmax(y))
        if y[k] > best:
            best, where = float(y[k]), (c, k)
    return (best, where) if return_argmax else best


def dbtp(tp):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(tp)


def sum_abs_taps(h, F):
    """max over the phases of sum |h|: the gain bound of the interpolator."""
    h = np.abs(np.asarray(h, dtype=np.float64))
    return max(float(h[p::F].sum()) for p in range(F))


def true_peak_bound(h, F, xmax):
    """|TP_fp32 - TP_f64| allowed: an output is a sum of at most 12 fused multiply-adds (at F = 2 two such sums and one addition),
    each rounding at most 2^-24 of a partial sum that never exceeds sum |h| max |x|: 13 * 2^-24 * sum |h| * max |x|."""
    return 13.0 * 2.0 ** -24 * sum_abs_taps(h, F) * xmax


# ---- short-term loudness and range ------------------------------------------------------------------------------------------------
def segment_step(rate):
    return R.block_bounds(1, rate)[0]


def num_short_term(n, rate, H):
    return (n // segment_step(rate) - SHORT_SEGMENTS) // H + 1


def short_term(x, rate, H):
    """x (channels, n) -> (E (NS,), l (NS,)) float64: energy and loudness of every 3 s window of the signal filtered once."""
    y = np.asarray(x, dtype=np.float64).copy()
    for b, a in R.k_weighting(rate):
        for c in range(y.shape[0]):
            y[c] = R._lfilter(b, a, y[c])
    step = segment_step(rate)
    G = np.array(R.GAINS[:y.shape[0]])
    E = np.zeros(num_short_term(y.shape[1], rate, H))
    for k in range(len(E)):
        lo, hi = R.block_bounds(k * H, rate)[0], R.block_bounds(k * H + SHORT_SEGMENTS, rate)[0]
        assert hi - lo == SHORT_SEGMENTS * step and hi <= y.shape[1]
        E[k] = float(np.sum(G * np.sum(np.square(y[:, lo:hi]), axis=1) / (SHORT_SEGMENTS * step)))
    with np.errstate(divide="ignore"):
        return E, -0.691 + 10.0 * np.log10(E)


def range_gates(l):
    """(absolutely gated indices, relative threshold, surviving indices) from short-term loudness alone (E = 10^((l + 0.691) / 10))."""
    l = np.asarray(l, dtype=np.float64)
    e = 10.0 ** ((l + 0.691) / 10.0)
    a = [k for k in range(len(l)) if l[k] >= -70.0]
    with np.errstate(divide="ignore"):
        gamma = -0.691 + 10.0 * np.log10(np.mean(e[a]) if a else 0.0) - 20.0
    return a, float(gamma), [k for k in a if l[k] >= gamma]


def loudness_range(E):
    """E (NS,) -> (LRA, l(lo), l(hi), absolute set, survivors): Tech 3342 with the percentile indices in integers."""
    E = np.asarray(E, dtype=np.float64)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(E)
        a = [k for k in range(len(E)) if l[k] >= -70.0]
        gamma = -0.691 + 10.0 * np.log10(np.mean(E[a]) if a else 0.0) - 20.0
    f = [k for k in a if l[k] >= gamma]
    m = len(f)
    if m == 0:
        return 0.0, float("nan"), float("nan"), a, f
    s = np.sort(E[f])
    lo, hi = s[((m - 1) * 10 + 50) // 100], s[((m - 1) * 95 + 50) // 100]
    l_lo, l_hi = -0.691 + 10.0 * math.log10(lo), -0.691 + 10.0 * math.log10(hi)
    return l_hi - l_lo, l_lo, l_hi, a, f


def range_margins(l):
    """(distance of the nearest window to the relative gate, to the absolute gate)."""
    l = np.asarray(l, dtype=np.float64)
    fin = l[np.isfinite(l)]
    a, gamma, _ = range_gates(l)
    m_abs = float(np.min(np.abs(fin - (-70.0)))) if len(fin) else np.inf
    m_rel = float(np.min(np.abs(fin - gamma))) if a and len(fin) else np.inf
    return m_rel, m_abs


# ---- the calls --------------------------------------------------------------------------------------------------------------------
def lib_factor(L, rate):
    """``mst_true_peak_factor`` -> 4, 2, or 0 when it refuses (a status; the factor comes through a host pointer)."""
    from mst import _cabi

    out = ctypes.c_int32(-7)
    try:
        L.mst_true_peak_factor(rate, ctypes.byref(out))
    except _cabi.AbiError:
        assert out.value == 0
        return 0
    assert out.value in (2, 4)
    return out.value


def lib_taps(L, F):
    h = (ctypes.c_float * TAPS)()
    L.mst_true_peak_coefficients(F, h)
    return np.array(h[:], dtype=np.float32)


def count_short_term(L, n, rate, H):
    from mst import _cabi

    out = ctypes.c_int32(-7)
    try:
        L.mst_loudness_num_short_term(n, rate, H, ctypes.byref(out))
    except _cabi.AbiError:
        assert out.value == 0
        return 0
    assert out.value > 0
    return out.value


GUARD = 64


def guarded(shape, device, fill=float("nan")):
    """An output buffer with GUARD floats of 12345 in front of it and behind it -> (the whole buffer, the view to hand over)."""
    count = int(np.prod(shape))
    buf = torch.full((count + 2 * GUARD,), 12345.0, device=device)
    buf[GUARD:GUARD + count] = fill
    return buf, buf[GUARD:GUARD + count].view(*shape)


def guards_intact(buf):
    return bool((buf[:GUARD] == 12345.0).all() and (buf[-GUARD:] == 12345.0).all())


def call_true_peak(L, x, F, per_channel=True, fill=float("nan")):
    """x fp32 tensor (rows, channels, n), any row / channel stride -> (true peak (rows), channel peaks (rows, channels) | None), linear.
    Workspace filled with `fill`, outputs guarded."""
    rows, chs, n = x.shape
    assert x.stride(2) == 1 or n == 1
    nbytes = L.mst_true_peak_workspace_bytes(rows, chs, n, F)
    assert nbytes > 0
    ws = torch.full((nbytes // 4 + 1,), fill, device=x.device)
    pb, peak = guarded((rows,), x.device)
    cb, chan = guarded((rows, chs), x.device) if per_channel else (None, None)
    L.mst_true_peak(x, rows, chs, n, x.stride(0), x.stride(1), F, peak, chan, ws, nbytes, None)
    assert guards_intact(pb) and (cb is None or guards_intact(cb))
    return peak.clone(), None if chan is None else chan.clone()


def call_range(L, x, rate, tables, H, fill=float("nan"), want=("short", "bounds", "lufs", "blocks")):
    """-> dict(range (rows), short (rows, NS), bounds (rows, 2), lufs (rows), blocks (rows, NB)) of tensors; optional ones None."""
    rows, chs, n = x.shape
    ns = count_short_term(L, n, rate, H)
    nbytes = L.mst_loudness_range_workspace_bytes(rows, chs, n, rate, H)
    nb = L.mst_loudness_num_blocks(n, rate)
    assert ns > 0 and nbytes > 0 and nb > 0
    ws = torch.full((nbytes // 8 + 1,), fill, dtype=torch.float64, device=x.device)
    bufs, out = {}, {}
    for name, shape in (("range", (rows,)), ("short", (rows, ns)), ("bounds", (rows, 2)), ("lufs", (rows,)), ("blocks", (rows, nb))):
        bufs[name], out[name] = guarded(shape, x.device) if name == "range" or name in want else (None, None)
    L.mst_loudness_range(x, rows, chs, n, x.stride(0), x.stride(1), rate, tables, H, out["short"], out["range"], out["bounds"],
                         out["lufs"], out["blocks"], ws, nbytes, None)
    assert all(b is None or guards_intact(b) for b in bufs.values())
    return {k: None if v is None else v.clone() for k, v in out.items()}
