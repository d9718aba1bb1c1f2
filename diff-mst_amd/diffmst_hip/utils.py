"""``mst.utils`` - the helper on the hot path (reference mst/utils.py:14-29)."""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch.autograd.function import once_differentiable

from . import _hip


class _PeakNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _hip.require_cuda(x)
        lib = _hip.lib()
        if x.dim() != 3:
            raise ValueError("expected a (bs, chs, seq_len) tensor")
        shape = x.shape
        xc = x.float().contiguous()
        if shape[1] != 2:
            # the peak runs over (channels, time) of a batch item, so any channel count is the stereo kernel on a
            # (bs, 2, chs*n/2) view of the same memory (reference mst/system.py:390-391 normalises a MONO sum)
            flat = xc.view(shape[0], -1)
            if flat.size(1) % 2:  # odd element count: one zero sample of padding leaves the peak unchanged
                flat = torch.nn.functional.pad(flat, (0, 1))
            xc = flat.view(shape[0], 2, flat.size(1) // 2)
        bs, _, n = xc.shape
        dev = xc.device
        nbytes = lib.mst_peak_normalize_workspace_bytes(bs, n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        y = torch.empty_like(xc)
        with _hip.launch_on(dev) as st:
            lib.mst_peak_normalize_forward(xc, y, bs, n, ws, nbytes, st)
        ctx.save_for_backward(xc, ws)
        ctx.nbytes = nbytes
        ctx.shape = shape
        return y.view(shape[0], -1)[:, : shape[1] * shape[2]].reshape(shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xc, ws = ctx.saved_tensors
        lib = _hip.lib()
        bs, _, n = xc.shape
        dev = xc.device
        g = g.float().contiguous().view(ctx.shape[0], -1)
        if g.size(1) != 2 * n:
            g = torch.nn.functional.pad(g, (0, 2 * n - g.size(1)))
        g = g.contiguous().view(xc.shape)
        dx = torch.empty_like(xc)
        with _hip.launch_on(dev) as st:
            lib.mst_peak_normalize_backward(xc, g, dx, bs, n, ws, ctx.nbytes, st)
        shape = ctx.shape
        return dx.view(shape[0], -1)[:, : shape[1] * shape[2]].reshape(shape)


def batch_stereo_peak_normalize(x: torch.Tensor):
    """Normalize a batch of mixes ``(bs, chs, seq_len)`` by their peak value over (chs, seq_len), per batch item."""
    return _PeakNormalize.apply(x)


# ------------------------------------------------------------------------------------------------
# Integrated loudness on the device (mst_loudness.hip).  BS.1770-4 as pyloudnorm.Meter computes it with its defaults;
# PARITY UNPINNED: restated from pyloudnorm's published source, never run against the package.
# ------------------------------------------------------------------------------------------------
_LOUDNESS_TABLES = {}


def _loudness_tables(device, sample_rate):
    """Block boundaries, K-weighting coefficients and transition-matrix powers: built once per (device, rate)."""
    lib = _hip.lib()
    return _hip.device_tables(_LOUDNESS_TABLES, (str(device), int(sample_rate)), device, lib.mst_loudness_tables_bytes,
                              lib.mst_loudness_init_tables, int(sample_rate), dtype=torch.uint8,
                              unsupported=f"unsupported sample rate {sample_rate} (the device meter needs at least 20500 Hz)")


def _forward_only(x, what):
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError(f"{what} is forward-only (the reference never differentiates through the loudness meter); "
                                  "detach the input or call it under torch.no_grad()")


def _as_rows(x):
    """``(..., channels, n)`` -> a ``(rows, channels, n)`` fp32 view with unit sample stride (copies only when it has to)."""
    if x.dim() < 2:
        raise ValueError("expected a (..., channels, n_samples) tensor")
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(-1) != 1 and x.shape[-1] > 1:
        x = x.contiguous()
    return x.reshape(-1, x.shape[-2], x.shape[-1])  # a view whenever the leading dimensions collapse


def _check_audio(channels, n, sample_rate):
    """pyloudnorm's ``valid_audio`` checks with its messages; raised before anything touches the device."""
    if channels > 5:
        raise ValueError("Audio must have five channels or less.")
    if n < 0.4 * sample_rate:
        raise ValueError("Audio must have length greater than the block size.")


def _meter(x3, sample_rate, return_blocks):
    lib = _hip.lib()
    rows, chs, n = x3.shape
    dev = x3.device
    _check_audio(chs, n, sample_rate)
    nblocks = lib.mst_loudness_num_blocks(n, int(sample_rate)) if rows > 0 and chs > 0 else 0
    tables = _loudness_tables(dev, sample_rate)
    nbytes = lib.mst_loudness_workspace_bytes(rows, chs, n, int(sample_rate))
    if nbytes == 0 or nblocks == 0:
        raise ValueError(f"unsupported loudness call: rows={rows}, channels={chs}, n_samples={n}, sample_rate={sample_rate}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lufs = torch.empty(rows, dtype=torch.float32, device=dev)
    blocks = torch.empty(rows, nblocks, dtype=torch.float32, device=dev) if return_blocks else None
    with _hip.launch_on(dev) as st:
        lib.mst_loudness_integrated(x3, rows, chs, n, x3.stride(0), x3.stride(1), int(sample_rate), tables, lufs, blocks, ws, nbytes, st)
    return lufs, blocks


def integrated_loudness(x: torch.Tensor, sample_rate: int = 44100, return_blocks: bool = False):
    """Integrated loudness (LUFS) of ``x (..., channels, n)`` on the device -> tensor of shape ``(...)``; with
    ``return_blocks`` also the loudness of every 0.4 s gating block, ``(..., num_blocks)``.  Channel weights 1, 1, 1, 1.41, 1.41;
    ``-inf`` where no block passes the gates.  Nothing is read back: the call never synchronises with the host."""
    x3 = _as_rows(x)
    _check_audio(x3.shape[1], x3.shape[2], sample_rate)
    _hip.require_cuda(x)
    _forward_only(x, "integrated_loudness")
    lufs, blocks = _meter(x3, sample_rate, return_blocks)
    lead = x.shape[:-2]
    if return_blocks:
        return lufs.view(lead), blocks.view(*lead, blocks.shape[-1])
    return lufs.view(lead)


_BLOCK_STEP = {}


def _block_step(sample_rate):
    """Samples between two gating-block boundaries when the meter's table ``int(0.4 * (k * 0.25) * rate)`` is equally spaced over all
    of its 4096 entries (44100, 48000, 22050, 32000, 96000, 88200, 24000 Hz ...); ``ValueError`` for any other rate."""
    if isinstance(sample_rate, bool) or sample_rate != int(sample_rate):
        raise ValueError(f"sample_rate must be a whole number of Hz, got {sample_rate!r}")
    rate = int(sample_rate)
    step = _BLOCK_STEP.get(rate)
    if step is None:
        step = int(0.4 * (1 * 0.25) * rate)
        if rate < 20500 or any(int(0.4 * (k * 0.25) * rate) != k * step for k in range(4096)):
            step = 0
        _BLOCK_STEP[rate] = step
    if not step:
        raise ValueError(f"unsupported sample rate {sample_rate}: the windowed meter needs gating blocks that start every rate / 10 "
                         "samples exactly (44100, 48000, 22050, 32000, 96000, 88200, 24000 Hz do)")
    return step


def loudness_window_grid(n_samples, length, hop=None, sample_rate=44100):
    """The host arithmetic of ``windowed_loudness``: ``(window_blocks W, hop_blocks H, starts)`` for a signal of ``n_samples``.  With
    ``step = rate / 10``: the signal has ``NB = n_samples // step - 3`` complete gating blocks, a window of ``length`` samples holds
    ``W = floor((length - 0.4 rate) / (0.1 rate)) + 1`` of them, ``hop`` (samples, a multiple of ``step``, default ``step``) is ``H``
    blocks, there are ``NW = (NB - W) // H + 1`` windows and window ``w`` starts at sample ``int(0.4 * (w H * 0.25) * rate)``, the
    boundary of its first block.  Everything that cannot be metered is a ``ValueError`` here, before any device call."""
    step = _block_step(sample_rate)
    rate = int(sample_rate)
    n_samples, length = int(n_samples), int(length)
    if length < 0.4 * rate:
        raise ValueError(f"a window must hold one gating block: length >= {4 * step} samples at {rate} Hz, got {length}")
    hop = step if hop is None else hop
    if isinstance(hop, bool) or hop != int(hop) or int(hop) < step or int(hop) % step:
        raise ValueError(f"hop must be a positive multiple of rate / 10 = {step} samples, got {hop!r}")
    if n_samples < 0.4 * rate:
        raise ValueError("Audio must have length greater than the block size.")
    W, H, NB = length // step - 3, int(hop) // step, n_samples // step - 3
    if NB > 4092:
        raise ValueError(f"{n_samples} samples are {NB} gating blocks; the device meter takes 4092 ({4095 * step} samples) at most")
    if W > NB:
        raise ValueError(f"a window of {length} samples does not fit into the {n_samples} samples of the signal")
    return W, H, [int(0.4 * ((w * H) * 0.25) * rate) for w in range((NB - W) // H + 1)]


def windowed_loudness(x: torch.Tensor, length: int, hop=None, sample_rate: int = 44100):
    """Gated loudness (LUFS) of every window of ``length`` samples of ``x (..., channels, n)``, ``hop`` samples apart (a multiple of
    ``rate / 10``, which is the default) -> ``(lufs (..., NW) fp32 on the device, starts)`` with ``starts`` the list of the windows'
    first samples, computed on the host (``loudness_window_grid``).  Nothing is read back from the device.

    The signal is K-weighted ONCE (``mst_loudness_windows``): a window's loudness is BS.1770 gating - absolute gate, relative gate, both
    within the window - over the complete 0.4 s gating blocks inside ``[start, start + length)``, with the filter warm at its start.
    That is the loudness of the window as a part of the song; ``integrated_loudness(x[..., start:start + length])`` filters the crop
    from rest and, unless ``length - 0.4 rate`` is a multiple of ``0.1 rate``, counts one clipped partial block more.
    ``-inf`` where no block of a window passes the gates.  Forward-only, like the meter."""
    x3 = _as_rows(x)
    if x3.shape[1] > 5:
        raise ValueError("Audio must have five channels or less.")
    W, H, starts = loudness_window_grid(x3.shape[2], length, hop, sample_rate)
    _hip.require_cuda(x)
    _forward_only(x, "windowed_loudness")
    lib = _hip.lib()
    rows, chs, n = x3.shape
    rate, dev = int(sample_rate), x3.device
    tables = _loudness_tables(dev, rate)
    nbytes = lib.mst_loudness_windows_workspace_bytes(rows, chs, n, rate, W, H)
    if nbytes == 0:
        raise ValueError(f"unsupported loudness call: rows={rows}, channels={chs}, n_samples={n}, sample_rate={sample_rate}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(rows, len(starts), dtype=torch.float32, device=dev)
    with _hip.launch_on(dev) as st:
        lib.mst_loudness_windows(x3, rows, chs, n, x3.stride(0), x3.stride(1), rate, tables, W, H, out, None, ws, nbytes, st)
    return out.view(*x.shape[:-2], len(starts)), starts


def loudness_normalize(x: torch.Tensor, target_lufs: float, sample_rate: int = 44100, floor_lufs=None):
    """``y = x * 10^((target_lufs - L) / 20)`` with ``L`` the integrated loudness of every ``(channels, n)`` item of
    ``x (..., channels, n)``, the gain formed on the device.  Returns ``(y, lufs (...), keep (...) bool)``, all on the device;
    items below ``floor_lufs`` (and silent ones, ``L = -inf``) have ``keep = False`` and come back as zeros."""
    x3 = _as_rows(x)
    _check_audio(x3.shape[1], x3.shape[2], sample_rate)
    _hip.require_cuda(x)
    _forward_only(x, "loudness_normalize")
    lufs, _ = _meter(x3, sample_rate, False)
    y, keep = _apply_loudness_gain(x3, lufs, target_lufs, floor_lufs)
    lead = x.shape[:-2]
    return y.view(x.shape), lufs.view(lead), keep.view(lead)


def _apply_loudness_gain(x3, lufs, target_lufs, floor_lufs):
    lib = _hip.lib()
    rows, chs, n = x3.shape
    dev = x3.device
    y = torch.empty(rows, chs, n, dtype=torch.float32, device=dev)
    keep = torch.empty(rows, dtype=torch.uint8, device=dev)
    floor = float("-inf") if floor_lufs is None else float(floor_lufs)
    with _hip.launch_on(dev) as st:
        lib.mst_loudness_normalize(x3, y, lufs, rows, chs, n, x3.stride(0), x3.stride(1), float(target_lufs), floor, keep, st)
    return y, keep.bool()


# ------------------------------------------------------------------------------------------------
# The rest of a delivery meter (mst_truepeak.hip, k_loud_range): true peak, short-term and momentary loudness, loudness
# range, and a normalisation that respects a true-peak ceiling.  PARITY UNPINNED: written from BS.1770-4 Annex 2 and EBU Tech
# 3341 / 3342, never run against another meter.  All forward-only, nothing is read back from the device.
# ------------------------------------------------------------------------------------------------
def true_peak_factor(sample_rate):
    """Oversampling factor of the true-peak meter: 4 below 96000 Hz, 2 below 192000 Hz; ``ValueError`` for any other rate."""
    if isinstance(sample_rate, bool) or sample_rate != int(sample_rate) or int(sample_rate) <= 0:
        raise ValueError(f"sample_rate must be a positive whole number of Hz, got {sample_rate!r}")
    rate = int(sample_rate)
    if rate >= 192000:
        raise ValueError(f"unsupported sample rate {sample_rate}: the true-peak meter oversamples rates below 192000 Hz only")
    return 4 if rate < 96000 else 2


def _true_peak_linear(x3, sample_rate, per_channel=False, sample_peak=False):
    """``(rows, channels, n)`` -> (true peak (rows), per channel (rows, channels) or None, sample peak max |x| (rows) or None), LINEAR
    fp32 on the device, all from one pass."""
    factor = true_peak_factor(sample_rate)
    lib = _hip.lib()
    rows, chs, n = x3.shape
    dev = x3.device
    nbytes = lib.mst_true_peak_workspace_bytes(rows, chs, n, factor)
    if nbytes == 0:
        raise ValueError(f"unsupported true-peak call: rows={rows}, channels={chs}, n_samples={n}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    peak = torch.empty(rows, dtype=torch.float32, device=dev)
    chan = torch.empty(rows, chs, dtype=torch.float32, device=dev) if per_channel else None
    sample = torch.empty(rows, dtype=torch.float32, device=dev) if sample_peak else None
    with _hip.launch_on(dev) as st:
        lib.mst_true_peak_sample(x3, rows, chs, n, x3.stride(0), x3.stride(1), factor, peak, chan, sample, ws, nbytes, st)
    return peak, chan, sample


def _check_true_peak(x3, sample_rate):
    true_peak_factor(sample_rate)
    if x3.shape[2] < 1 or x3.shape[0] * x3.shape[1] < 1:
        raise ValueError("true_peak needs at least one sample of at least one channel")
    if x3.shape[0] * x3.shape[1] > 65535:
        raise ValueError("true_peak takes 65535 signals (items x channels) per call at most")


def true_peak(x: torch.Tensor, sample_rate: int = 44100, per_channel: bool = False):
    """True peak (dBTP, BS.1770-4 Annex 2) of every ``(channels, n)`` item of ``x (..., channels, n)`` -> ``(...)``, or
    ``(..., channels)`` with ``per_channel``: ``20 log10`` of the largest magnitude of the signal interpolated 4 times (2 times from
    96 kHz) by a 49-tap Hann-windowed sinc, the tail after the last sample included.  ``-inf`` for silence, NaN for an item that holds
    a NaN.  The interpolated signal is never written; a last-dimension crop is read in place."""
    if x.dim() >= 2 and x.numel() == 0:
        raise ValueError("true_peak needs at least one sample of at least one channel")
    x3 = _as_rows(x)
    _check_true_peak(x3, sample_rate)
    _hip.require_cuda(x)
    _forward_only(x, "true_peak")
    peak, chan, _ = _true_peak_linear(x3, sample_rate, per_channel)
    if per_channel:
        return (20.0 * torch.log10(chan)).view(*x.shape[:-1])
    return (20.0 * torch.log10(peak)).view(x.shape[:-2])


def short_term_grid(n_samples, hop=None, sample_rate=44100):
    """The host arithmetic of ``short_term_loudness``: ``(hop_segments H, starts)``.  With ``step = rate / 10`` the signal has
    ``NSEG = n_samples // step`` segments, a short-term window is 30 of them (3 s), ``hop`` (samples, a multiple of ``step`` of at
    most 30, default ``10 step`` = 1 s) is ``H`` segments and there are ``(NSEG - 30) // H + 1`` windows, window ``k`` starting at sample
    ``k H step``.  Everything that cannot be metered is a ``ValueError`` here, before any device call."""
    step = _block_step(sample_rate)
    n_samples = int(n_samples)
    hop = 10 * step if hop is None else hop
    if isinstance(hop, bool) or hop != int(hop) or int(hop) < step or int(hop) % step or int(hop) > 30 * step:
        raise ValueError(f"hop must be a multiple of rate / 10 = {step} samples between {step} and {30 * step}, got {hop!r}")
    nseg = n_samples // step
    if nseg < 30:
        raise ValueError(f"short-term loudness needs 3 s of audio ({30 * step} samples at {int(sample_rate)} Hz), got {n_samples}")
    if nseg - 3 > 4092:
        raise ValueError(f"{n_samples} samples are {nseg - 3} gating blocks; the device meter takes 4092 ({4095 * step} samples) at most")
    H = int(hop) // step
    return H, [k * H * step for k in range((nseg - 30) // H + 1)]


def _range_call(x3, sample_rate, H, ns, want_short, want_bounds, want_blocks):
    """One K-weighting pass and the range launch -> (range (rows), short-term (rows, NS) | None, bounds (rows, 2) | None,
    lufs (rows), block loudness (rows, NB) | None)."""
    lib = _hip.lib()
    rows, chs, n = x3.shape
    rate, dev = int(sample_rate), x3.device
    tables = _loudness_tables(dev, rate)
    nbytes = lib.mst_loudness_range_workspace_bytes(rows, chs, n, rate, H)
    nblocks = lib.mst_loudness_num_blocks(n, rate)
    if nbytes == 0 or nblocks == 0:
        raise ValueError(f"unsupported loudness call: rows={rows}, channels={chs}, n_samples={n}, sample_rate={sample_rate}")
    f32 = dict(dtype=torch.float32, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lra, lufs = torch.empty(rows, **f32), torch.empty(rows, **f32)
    short = torch.empty(rows, ns, **f32) if want_short else None
    bounds = torch.empty(rows, 2, **f32) if want_bounds else None
    blocks = torch.empty(rows, nblocks, **f32) if want_blocks else None
    with _hip.launch_on(dev) as st:
        lib.mst_loudness_range(x3, rows, chs, n, x3.stride(0), x3.stride(1), rate, tables, H, short, lra, bounds, lufs, blocks, ws,
                               nbytes, st)
    return lra, short, bounds, lufs, blocks


def _range_rows(x, hop, sample_rate, what):
    x3 = _as_rows(x)
    if x3.shape[1] > 5:
        raise ValueError("Audio must have five channels or less.")
    H, starts = short_term_grid(x3.shape[2], hop, sample_rate)
    _hip.require_cuda(x)
    _forward_only(x, what)
    return x3, H, starts


def short_term_loudness(x: torch.Tensor, hop=None, sample_rate: int = 44100):
    """Short-term loudness (LUFS, ungated, 3 s windows) of ``x (..., channels, n)`` -> ``(lufs (..., NS) on the device, starts)``;
    ``hop`` in samples, a multiple of ``rate / 10`` (default one second), ``starts`` the windows' first samples (``short_term_grid``).
    The song is K-weighted once and the filter is warm at a window's start; ``-inf`` for a silent window."""
    x3, H, starts = _range_rows(x, hop, sample_rate, "short_term_loudness")
    _, short, _, _, _ = _range_call(x3, sample_rate, H, len(starts), True, False, False)
    return short.view(*x.shape[:-2], len(starts)), starts


def momentary_loudness(x: torch.Tensor, sample_rate: int = 44100):
    """Momentary loudness (LUFS, ungated, 0.4 s windows every 0.1 s) of ``x (..., channels, n)`` -> ``(..., num_blocks)``: the block
    loudness the meter already forms (``integrated_loudness(x, rate, return_blocks=True)[1]``)."""
    return integrated_loudness(x, sample_rate, return_blocks=True)[1]


def loudness_range(x: torch.Tensor, sample_rate: int = 44100, hop=None, return_bounds: bool = False):
    """Loudness range (LU, EBU Tech 3342) of every item of ``x (..., channels, n)`` -> ``(...)``: the spread between the 10th and the
    95th percentile of the short-term loudness that passes an absolute gate at -70 LUFS and a relative gate 20 LU below the gated
    mean.  With ``return_bounds`` also ``(..., 2)``, the two percentiles in LUFS (NaN where no window survives; the range is 0
    there).  ``hop`` as in ``short_term_loudness``; Tech 3342 asks for at least 2 s of overlap, i.e. ``hop <= rate``."""
    x3, H, starts = _range_rows(x, hop, sample_rate, "loudness_range")
    lra, _, bounds, _, _ = _range_call(x3, sample_rate, H, len(starts), False, return_bounds, False)
    lead = x.shape[:-2]
    return (lra.view(lead), bounds.view(*lead, 2)) if return_bounds else lra.view(lead)


class LoudnessReport(NamedTuple):
    """What a delivery meter shows, every field a device tensor of the input's leading shape: LUFS, LU, LUFS, LUFS, dBTP, dBFS."""
    integrated: torch.Tensor
    loudness_range: torch.Tensor
    momentary_max: torch.Tensor
    short_term_max: torch.Tensor
    true_peak: torch.Tensor
    sample_peak: torch.Tensor


def meter_report(x: torch.Tensor, sample_rate: int = 44100) -> LoudnessReport:
    """The meter readings of every item of ``x (..., channels, n)`` from one K-weighting pass, one range launch (short-term hop of one
    second) and the true-peak launches; the maxima are ``amax`` of the momentary and short-term series."""
    x3, H, starts = _range_rows(x, None, sample_rate, "meter_report")
    _check_true_peak(x3, sample_rate)
    lra, short, _, lufs, blocks = _range_call(x3, sample_rate, H, len(starts), True, False, True)
    peak, _, sample = _true_peak_linear(x3, sample_rate, sample_peak=True)
    lead = x.shape[:-2]
    sample = 20.0 * torch.log10(sample)
    return LoudnessReport(lufs.view(lead), lra.view(lead), blocks.amax(dim=1).view(lead), short.amax(dim=1).view(lead),
                          (20.0 * torch.log10(peak)).view(lead), sample.view(lead))


def loudness_normalize_limited(x: torch.Tensor, target_lufs: float, ceiling_dbtp: float = -1.0, sample_rate: int = 44100,
                               floor_lufs=None):
    """``loudness_normalize`` with the gain capped so that the true peak of the result stays at or below ``ceiling_dbtp``:
    ``g = min(10^((target_lufs - L) / 20), 10^(ceiling_dbtp / 20) / TP)``, formed on the device.  Returns ``(y, lufs (...), keep (...)
    bool, gain_db (...), true_peak (...) dBTP of the input)``; an item the cap took hold of ends ``target - L - gain_db`` LU below
    the target.  Items below ``floor_lufs`` and silent ones have ``keep = False``, come back as zeros and have ``gain_db = -inf``."""
    x3 = _as_rows(x)
    _check_audio(x3.shape[1], x3.shape[2], sample_rate)
    _check_true_peak(x3, sample_rate)
    _hip.require_cuda(x)
    _forward_only(x, "loudness_normalize_limited")
    lufs, _ = _meter(x3, sample_rate, False)
    peak, _, _ = _true_peak_linear(x3, sample_rate)
    lib = _hip.lib()
    rows, chs, n = x3.shape
    dev = x3.device
    y = torch.empty(rows, chs, n, dtype=torch.float32, device=dev)
    keep = torch.empty(rows, dtype=torch.uint8, device=dev)
    gain = torch.empty(rows, dtype=torch.float32, device=dev)
    floor = float("-inf") if floor_lufs is None else float(floor_lufs)
    with _hip.launch_on(dev) as st:
        lib.mst_loudness_normalize_limited(x3, y, lufs, peak, rows, chs, n, x3.stride(0), x3.stride(1), float(target_lufs), floor,
                                           float(ceiling_dbtp), gain, keep, st)
    lead = x.shape[:-2]
    return y.view(x.shape), lufs.view(lead), keep.bool().view(lead), gain.view(lead), (20.0 * torch.log10(peak)).view(lead)


class LoudnessMeter:
    """Drop-in for ``pyloudnorm.Meter(rate)`` where only ``integrated_loudness`` is used (defaults: K-weighting, 0.4 s blocks):
    ``integrated_loudness(data)`` takes what pyloudnorm takes - a numpy array or host tensor ``(n,)`` / ``(n, channels)`` -
    runs the device meter on it and returns a Python ``float``.  ``run_diffmst(..., loudness_fn=LoudnessMeter(44100)
    .integrated_loudness)`` works on a machine without pyloudnorm."""

    def __init__(self, rate: int):
        self.rate = int(rate)

    def integrated_loudness(self, data) -> float:
        x = torch.as_tensor(data)
        if x.dim() == 1:
            x = x.unsqueeze(1)
        if x.dim() != 2:
            raise ValueError("expected (n_samples,) or (n_samples, channels) audio")
        if not x.is_floating_point():
            raise ValueError("Data must be floating point.")  # pyloudnorm's message
        _check_audio(x.shape[1], x.shape[0], self.rate)
        dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
        x = x.detach().to(device=dev, dtype=torch.float32).t().contiguous()  # (channels, n)
        return float(integrated_loudness(x, self.rate).item())


# ------------------------------------------------------------------------------------------------
# Sample-rate conversion on the device (mst_resample.hip).  torchaudio.functional.resample with its defaults (sinc_interp_hann,
# lowpass_filter_width 6, rolloff 0.99); PARITY UNPINNED: restated from torchaudio's published source, never run against the
# package.
# ------------------------------------------------------------------------------------------------
_RESAMPLE_TABLES = {}


def _int_rate(value, name):
    """Sample rates are ints or integral floats (torchaudio converts both with int()); anything else is refused."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or value != value or value in (float("inf"), float("-inf")):
        raise ValueError(f"{name} must be an integer sample rate, got {value!r}")
    if float(value) != int(value):
        raise ValueError(f"{name} must be an integer sample rate, got {value!r} (fractional rates are not supported)")
    if int(value) <= 0:
        raise ValueError(f"{name} must be positive, got {value!r}")
    return int(value)


def _resample_tables(device, orig_freq, new_freq):
    """Both coefficient tables (forward and adjoint) of a ratio: built once per (device, o, n)."""
    import math

    g = math.gcd(orig_freq, new_freq)
    key = (str(device), orig_freq // g, new_freq // g)
    lib = _hip.lib()
    return _hip.device_tables(_RESAMPLE_TABLES, key, device, lib.mst_resample_tables_bytes, lib.mst_resample_init_tables, orig_freq, new_freq,
                              dtype=torch.uint8,
                              unsupported=f"unsupported resampling ratio {orig_freq} -> {new_freq}: reduced to {key[1]}:{key[2]}, the device "
                                          "resampler takes reduced rates up to 1024 and at most 132 taps per output sample")


def _time_rows(x):
    """``(..., time)`` -> a ``(rows, time)`` fp32 view with unit sample stride (copies only when it has to)."""
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(-1) != 1:
        x = x.contiguous()
    return x.reshape(-1, x.shape[-1])  # a view whenever the leading dimensions collapse (a last-dimension slice does)


class _Resample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, orig_freq, new_freq):
        lib = _hip.lib()
        dev = x.device
        tables = _resample_tables(dev, orig_freq, new_freq)
        rows = _time_rows(x.detach())
        n_rows, n = rows.shape
        n_out = lib.mst_resample_out_samples(n, orig_freq, new_freq)
        if n_out <= 0:
            raise ValueError(f"unsupported resample call: {n} samples, {orig_freq} -> {new_freq}")
        y = torch.empty(n_rows, n_out, dtype=torch.float32, device=dev)
        if n_rows:
            with _hip.launch_on(dev) as st:
                lib.mst_resample_forward(rows, n_rows, n, rows.stride(0), orig_freq, new_freq, tables, y, st)
        ctx.rates = (orig_freq, new_freq)
        ctx.in_shape, ctx.in_dtype = x.shape, x.dtype
        return y.view(*x.shape[:-1], n_out).to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lib = _hip.lib()
        orig_freq, new_freq = ctx.rates
        dev = g.device
        n = ctx.in_shape[-1]
        g2 = g.float().contiguous().view(-1, g.shape[-1])
        gx = torch.empty(g2.shape[0], n, dtype=torch.float32, device=dev)
        if g2.shape[0]:
            tables = _resample_tables(dev, orig_freq, new_freq)
            with _hip.launch_on(dev) as st:
                lib.mst_resample_backward(g2, g2.shape[0], n, orig_freq, new_freq, tables, gx, st)
        return gx.view(ctx.in_shape).to(ctx.in_dtype), None, None


def resample(waveform: torch.Tensor, orig_freq, new_freq):
    """``torchaudio.functional.resample(waveform, orig_freq, new_freq)`` (defaults: Hann-windowed sinc interpolation, width 6,
    roll-off 0.99) of a device tensor ``(..., time)`` -> ``(..., ceil(time * new / orig))``, differentiable with respect to
    ``waveform``.  Equal rates return ``waveform`` itself.  The arithmetic is fp32 with coefficients evaluated in float64 on the
    host; other floating dtypes are converted and the result is cast back, so a float64 input is computed in fp32 here
    (torchaudio would compute it in float64).  A last-dimension slice of a wider buffer is read in place.  The output length is
    evaluated in integers (torchaudio: through a float32 tensor, one sample off in rare cases above 2^24 samples)."""
    orig_freq, new_freq = _int_rate(orig_freq, "orig_freq"), _int_rate(new_freq, "new_freq")
    if not isinstance(waveform, torch.Tensor) or not waveform.is_floating_point():
        raise TypeError("resample expects a floating-point tensor (..., time)")
    if orig_freq == new_freq:
        return waveform
    _hip.require_cuda(waveform)
    if waveform.dim() < 1 or waveform.shape[-1] < 1:
        raise ValueError("expected a (..., time) tensor with at least one sample")
    _resample_tables(waveform.device, orig_freq, new_freq)  # an unsupported ratio raises before anything is launched
    return _Resample.apply(waveform, orig_freq, new_freq)


class Resample(torch.nn.Module):
    """``torchaudio.transforms.Resample(orig_freq, new_freq)`` with its default method: ``Resample(a, b)(x) = resample(x, a, b)``."""

    def __init__(self, orig_freq=16000, new_freq=16000):
        super().__init__()
        self.orig_freq, self.new_freq = _int_rate(orig_freq, "orig_freq"), _int_rate(new_freq, "new_freq")

    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        return resample(waveform, self.orig_freq, self.new_freq)

    def extra_repr(self):
        return f"orig_freq={self.orig_freq}, new_freq={self.new_freq}"


# ------------------------------------------------------------------------------------------------
# Inference driver (reference mst/utils.py:32-258): forward-only, batch 1, long songs
# ------------------------------------------------------------------------------------------------
ANALYSIS_LEN = 262144  # reference mst/utils.py:66
SAMPLE_RATE = 44100    # the rate the model, the meter and the console work at


def _default_loudness_fn(sample_rate=44100):
    """``pyloudnorm.Meter(44100).integrated_loudness`` like the reference (mst/utils.py:67, :93); the package is a host-side
    dependency of the reference, not part of the device path - inject ``loudness_fn`` where it is not installed."""
    try:
        import pyloudnorm as pyln
    except ImportError as e:  # fail loudly: there is no silent stand-in for BS.1770 loudness
        raise ImportError("run_diffmst needs pyloudnorm (reference requirements.txt), an explicit loudness_fn(ndarray (n, ch)) -> LUFS, "
                          "or loudness_fn=\"device\" for this package's own meter") from e
    return pyln.Meter(sample_rate).integrated_loudness


def run_diffmst(tracks: torch.Tensor, ref: torch.Tensor, model: torch.nn.Module, mix_console: torch.nn.Module,
                track_start_idx: int = 0, ref_start_idx: int = 0, loudness_fn=None, device=None, verbose: bool = False,
                track_sample_rate=44100, ref_sample_rate=44100):
    """Reference ``mst.utils.run_diffmst`` (mst/utils.py:32-173) on the HIP console.

    ``tracks (1, T, n)``, ``ref (1, 2, n_ref)`` (host or device tensors) ->
    ``(pred_mix (1, 2, n), track / fx-bus / master-bus parameter dictionaries)`` with the reference's steps: crop an analysis
    window of 262144 samples, normalise every track to -48 LUFS from its analysis crop (tracks below -80 LUFS are dropped),
    ONE parameter estimate ``model(analysis_tracks, analysis_ref)``, then console forwards over 262144-sample windows
    hopping by 131072, each faded with a periodic Hann window (the first window's first half held at 1) and overlap-added.

    Differences, all outside the arithmetic: the caller's ``tracks`` is not scaled in place (the reference's ``track *= ...``
    writes through a view); model and console windows run on ``device`` (default: the model's device if it is a GPU, else the
    current GPU; a model still on the host - what ``load_diffmst`` returns - is moved there with ``model.to(device)``) and
    ``pred_mix`` comes back on ``tracks.device``; ``loudness_fn(ndarray (n, 1)) -> float`` replaces the
    pyloudnorm meter where that package is absent (it is host-side in the reference too); ``loudness_fn="device"`` measures and
    normalises on the device instead (``integrated_loudness`` / ``loudness_normalize`` above - BS.1770 as pyloudnorm computes it,
    parity unpinned): one meter call over all tracks, and the only host read is the mask of the tracks that survive;
    ``track_sample_rate`` / ``ref_sample_rate`` other than 44100 convert that input to 44100 Hz on the device first (``resample``
    above - what the reference's scripts do with torchaudio before they call this function, scripts/run.py:78-79, :108-109), so
    ``track_start_idx`` / ``ref_start_idx`` index the 44100 Hz signals and ``pred_mix`` is returned at 44100 Hz."""
    if tracks.dim() != 3 or tracks.shape[0] != 1:
        raise ValueError("tracks must be (1, num_tracks, seq_len)")  # the reference's squeeze(0) / zeros(1, 2, n) fix bs = 1
    if loudness_fn is None:
        loudness_fn = _default_loudness_fn()
    if device is None:
        p = next(iter(model.parameters()), None) if isinstance(model, torch.nn.Module) else None
        device = p.device if p is not None and p.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if isinstance(model, torch.nn.Module):
        # load_diffmst returns the model on the host (map_location="cpu", like the reference, which runs there); this package has no
        # host path, so the model follows the audio onto the device - in place, like nn.Module.to
        if any(t.device != device for t in (*model.parameters(), *model.buffers())):
            model.to(device)
    out_device = tracks.device
    if _int_rate(track_sample_rate, "track_sample_rate") != SAMPLE_RATE:
        tracks = resample(tracks.detach().to(device=device, dtype=torch.float32), track_sample_rate, SAMPLE_RATE)
    if _int_rate(ref_sample_rate, "ref_sample_rate") != SAMPLE_RATE:
        ref = resample(ref.detach().to(device=device, dtype=torch.float32), ref_sample_rate, SAMPLE_RATE)
    n = tracks.shape[-1]
    if n >= ANALYSIS_LEN:
        analysis_tracks = tracks[..., track_start_idx:track_start_idx + ANALYSIS_LEN]
    else:
        analysis_tracks = tracks
    analysis_ref = ref[..., ref_start_idx:ref_start_idx + ANALYSIS_LEN] if ref.shape[-1] >= ANALYSIS_LEN else ref

    if isinstance(loudness_fn, str):
        if loudness_fn != "device":
            raise ValueError('loudness_fn must be a callable, None or "device"')
        norm_tracks, norm_analysis = _normalize_tracks_on_device(tracks, n, track_start_idx, device, verbose)
    else:
        norm_tracks, norm_analysis = _normalize_tracks_on_host(tracks, analysis_tracks, loudness_fn, device, verbose)
    return _mix_windows(out_device, norm_tracks, norm_analysis, analysis_ref, model, mix_console, device, n)


def _normalize_tracks_on_device(tracks, n, track_start_idx, device, verbose):
    """-48 LUFS from the analysis crop, -80 LUFS floor, all tracks in one meter call; the host reads the keep mask only."""
    dev_tracks = tracks.detach().to(device=device, dtype=torch.float32)[0].unsqueeze(1)  # (T, 1, n): rows = tracks, mono
    crop = dev_tracks[..., track_start_idx:track_start_idx + ANALYSIS_LEN] if n >= ANALYSIS_LEN else dev_tracks
    lufs, _ = _meter(crop, 44100, False)  # a last-dimension slice: strided rows, no copy
    y, keep = _apply_loudness_gain(dev_tracks, lufs, -48.0, -80.0)
    keep = keep.cpu()  # the number of surviving tracks shapes the model's input: the one inherent synchronisation
    if verbose:
        for t in (~keep).nonzero().flatten().tolist():
            print(f"Skipping track {t} due to low loudness {float(lufs[t])}.")
    if not bool(keep.any()):
        raise RuntimeError("every track is below -80 LUFS")
    y = y.view(1, -1, n)
    if not bool(keep.all()):
        y = y.index_select(1, keep.nonzero().flatten().to(device))
    norm_analysis = y[..., track_start_idx:track_start_idx + ANALYSIS_LEN].contiguous() if n >= ANALYSIS_LEN else y
    return y, norm_analysis


def _normalize_tracks_on_host(tracks, analysis_tracks, loudness_fn, device, verbose):
    # loudness-normalise to -48 LUFS (host side, like the reference: the meter works on numpy)
    keep, gains = [], []
    host_analysis = analysis_tracks.detach().float().cpu()
    for t in range(tracks.shape[1]):
        lufs_db = float(loudness_fn(host_analysis[0, t:t + 1].permute(1, 0).numpy()))
        if lufs_db < -80.0:
            if verbose:
                print(f"Skipping track {t} due to low loudness {lufs_db}.")
            continue
        keep.append(t)
        gains.append(10 ** ((-48 - lufs_db) / 20))
    if not keep:
        raise RuntimeError("every track is below -80 LUFS")  # the reference fails in torch.cat([]) here
    idx = torch.tensor(keep, device=tracks.device)
    g = torch.tensor(gains, dtype=torch.float32).view(1, -1, 1)
    norm_tracks = (tracks.detach().float().index_select(1, idx) * g.to(tracks.device)).to(device).contiguous()
    norm_analysis = (analysis_tracks.detach().float().index_select(1, idx) * g.to(tracks.device)).to(device).contiguous()
    return norm_tracks, norm_analysis


def _mix_windows(out_device, norm_tracks, norm_analysis, analysis_ref, model, mix_console, device, n):
    # ---- one parameter estimate from the analysis audio
    pred_track_params, pred_fx_bus_params, pred_master_bus_params = model(norm_analysis, analysis_ref.float().to(device))

    # ---- overlap-add of windowed console forwards
    pred_mix = torch.zeros(1, 2, n, dtype=torch.float32, device=device)
    window = torch.hann_window(ANALYSIS_LEN, device=device)
    first = window.clone()
    first[:ANALYSIS_LEN // 2] = 1.0
    dicts = None
    with torch.no_grad():
        for i in range(0, n, ANALYSIS_LEN // 2):
            win_tracks = norm_tracks[..., i:i + ANALYSIS_LEN]
            _, mix_w, *dicts = mix_console(
                win_tracks, pred_track_params, pred_fx_bus_params, pred_master_bus_params,
                use_track_input_fader=True, use_track_panner=True, use_track_eq=True, use_track_compressor=True,
                use_fx_bus=False, use_master_bus=True, use_output_fader=True,
            )
            m = mix_w.shape[-1]  # the last window is shorter: the reference pads it to 262144 before the fade
            pred_mix[..., i:i + m] += mix_w * (first if i == 0 else window)[:m]
    return (pred_mix.to(out_device), *dicts)


def load_diffmst(config_path: str, ckpt_path: str, map_location: str = "cpu"):
    """Reference ``mst.utils.load_diffmst`` (mst/utils.py:176-258): build the encoders, controller and console named by a
    training YAML (class paths resolved by import, so ``mst.modules.*`` means whatever ``mst`` is importable - this
    package's alias or a reference checkout after ``diffmst_hip.install()``), split a Lightning checkpoint's ``state_dict``
    by the ``model.track_encoder.`` / ``model.mix_encoder.`` / ``model.controller.`` / ``model.mix_console.`` prefixes and
    return ``(MixStyleTransferModel in eval mode, mix_console)``."""
    import yaml
    from importlib import import_module

    with open(config_path) as f:
        config = yaml.safe_load(f)

    def build(spec):
        module_path, class_name = spec["class_path"].rsplit(".", 1)
        return getattr(import_module(module_path), class_name)(**spec.get("init_args", {}))

    core = config["model"]["init_args"]["model"]
    sub = core["init_args"]
    parts = {name: build(sub[name]) for name in ("track_encoder", "mix_encoder", "controller")}
    mix_console = build(config["model"]["init_args"]["mix_console"])
    checkpoint = torch.load(ckpt_path, map_location=map_location)
    sd = checkpoint["state_dict"]
    for name, module in (*parts.items(), ("mix_console", mix_console)):
        prefix = f"model.{name}."
        module.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
    module_path, class_name = core["class_path"].rsplit(".", 1)
    model = getattr(import_module(module_path), class_name)(parts["track_encoder"], parts["mix_encoder"], parts["controller"])
    model.eval()
    return model, mix_console
