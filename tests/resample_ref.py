"""Restatement of ``torchaudio.functional.resample(x, orig_freq, new_freq)`` at its defaults (``sinc_interp_hann``,
``lowpass_filter_width=6``, ``rolloff=0.99``), written from the published source.

PARITY UNPINNED: torchaudio is not installed where this project is built and tested, so this file was never run against it.
What ties it to a resampler independently of the restatement is the closed form asserted in tests/test_resample_hostsim.py: a
997 Hz sine resampled equals the same sine sampled at the new rate (time alignment and gain).

(a) ``resample`` has literally torchaudio's shape: the dense ``(n, 1, K)`` kernel, ``F.pad``, ``F.conv1d(stride=o)``,
    transpose / reshape, truncate - in the dtype asked for (float32: the reference's own arithmetic; float64: the yardstick).
(b) ``forward_stats`` / ``adjoint_stats`` return the tap count and the largest absolute coefficient sum of the operator and of its
    adjoint, from which the tests derive their fp32 bounds.

TEST INFRASTRUCTURE: plain torch only.
"""
import functools
import math

import torch

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99


def reduced(orig_freq, new_freq):
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def out_samples(length, orig_freq, new_freq):
    """ceil(n L / o) in integers (torchaudio goes through a float32 tensor: may differ by one above 2^24; not imitated)."""
    o, n = reduced(orig_freq, new_freq)
    return (n * length + o - 1) // o


@functools.lru_cache(maxsize=None)
def sinc_kernel(orig_freq, new_freq, dtype=torch.float32):
    """torchaudio's ``_get_sinc_resample_kernel``: ``(kernel (n, 1, K) in `dtype`, width)``; float64 until the last cast."""
    o, n = reduced(orig_freq, new_freq)
    base = min(o, n) * ROLLOFF
    width = math.ceil(LOWPASS_FILTER_WIDTH * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None, None] / n + idx
    t = t * base
    t = t.clamp(-LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = torch.cos(t * math.pi / LOWPASS_FILTER_WIDTH / 2) ** 2
    t = t * math.pi
    scale = base / o
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t)
    kernels = kernels * window * scale
    return kernels.to(dtype), width


def resample(x, orig_freq, new_freq, dtype=torch.float32):
    """torchaudio's ``_apply_sinc_resample_kernel`` on a tensor ``(..., time)``, computed in `dtype` on the tensor's device (the
    tests use CPU tensors; tools/resample_bench.py times this dense formulation on the GPU)."""
    o, n = reduced(orig_freq, new_freq)
    if o == n:
        return x
    kernel, width = sinc_kernel(orig_freq, new_freq, dtype)
    kernel = kernel.to(x.device)
    shape = x.size()
    w = x.to(dtype).reshape(-1, shape[-1])
    length = w.shape[-1]
    w = torch.nn.functional.pad(w, (width, width + o))
    y = torch.nn.functional.conv1d(w[:, None], kernel, stride=o)
    y = y.transpose(1, 2).reshape(w.shape[0], -1)
    y = y[..., : out_samples(length, orig_freq, new_freq)]
    return y.view(shape[:-1] + y.shape[-1:])


def adjoint(grad_y, length, orig_freq, new_freq):
    """``A^T grad_y`` for inputs of `length` samples: torch autograd through (a) in float64."""
    x = torch.zeros(*grad_y.shape[:-1], length, dtype=torch.float64, requires_grad=True)
    y = resample(x, orig_freq, new_freq, torch.float64)
    (gx,) = torch.autograd.grad(y, x, grad_y.double())
    return gx


@functools.lru_cache(maxsize=None)
def forward_stats(orig_freq, new_freq):
    """``(T, S)``: the longest run of fp32 coefficients that are not exactly zero over the phases, and
    ``max_i sum_k |h[i][k]|``."""
    h = sinc_kernel(orig_freq, new_freq, torch.float32)[0][:, 0]  # (n, K)
    T = 0
    for row in h:
        nz = row.nonzero().flatten()
        T = max(T, int(nz[-1] - nz[0]) + 1)
    return T, float(h.double().abs().sum(1).max())


@functools.lru_cache(maxsize=None)
def adjoint_stats(orig_freq, new_freq):
    """The same two numbers for the adjoint: input residue ``r = (m + width) mod o`` is reached through the taps ``k = r + d o``;
    E = the longest run of output offsets ``i - d n`` with a non-zero coefficient, S = the largest column abs-sum."""
    o, n = reduced(orig_freq, new_freq)
    h = sinc_kernel(orig_freq, new_freq, torch.float32)[0][:, 0].double()
    K = h.shape[1]
    E, S = 0, 0.0
    for r in range(o):
        ks = torch.arange(r, K, o)
        col = h[:, ks]  # (n, d)
        S = max(S, float(col.abs().sum()))
        i, d = col.nonzero(as_tuple=True)
        v = i - d * n
        E = max(E, int(v.max() - v.min()) + 1)
    return E, S


def forward_bound(orig_freq, new_freq, max_abs=1.0):
    """|y_fp32 - y_f64| <= (T + 2) 2^-24 S max|x|: T fp32 fused multiply-adds (2^-24 relative each, on partial sums of at most
    S max|x|), one rounding of every coefficient to fp32 (2^-24 S max|x| in total) and one of the result."""
    T, S = forward_stats(orig_freq, new_freq)
    return (T + 2) * 2.0 ** -24 * S * max_abs


def adjoint_bound(orig_freq, new_freq, max_abs=1.0):
    E, S = adjoint_stats(orig_freq, new_freq)
    return (E + 2) * 2.0 ** -24 * S * max_abs


# ---- the cases tests/test_resample_hostsim.py and tests/test_resample_gpu.py share ---------------------------------------------
RATIOS = [(48000, 44100), (44100, 48000), (22050, 44100), (88200, 44100), (96000, 44100), (32000, 44100), (44100, 16000), (44100, 8000)]
# float64 restatement vs the same 997 Hz sine sampled at the new rate, 0.3 s, amplitude 1, first and last 10 ms left out: the
# pass-band ripple of the width-6 Hann-windowed sinc.  Measured: 4.57e-4 (48000->44100), 5.75e-4 (44100->48000),
# 1.46e-4 (22050->44100), 3.01e-4 (96000->44100), 3.97e-4 (44100->16000)
RESTATEMENT_VS_CLOSED_FORM = 6e-4
SINE_RATIOS = [(48000, 44100), (44100, 48000), (22050, 44100), (96000, 44100), (44100, 16000)]


def case_lengths(orig, new, frames_per_tile):
    """1; o - 1, o, o + 1; 2 width; one tile of input samples +- 1; 5003."""
    o, _ = reduced(orig, new)
    width = sinc_kernel(orig, new)[1]
    tile = frames_per_tile * o
    return sorted({v for v in (1, o - 1, o, o + 1, 2 * width, tile - 1, tile, tile + 1, 5003) if v >= 1})


def noise(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0


def sine_case(orig, new):
    n = int(round(0.3 * orig))
    x = torch.sin(2.0 * math.pi * 997.0 * torch.arange(n, dtype=torch.float64) / orig)
    n_out = out_samples(n, orig, new)
    want = torch.sin(2.0 * math.pi * 997.0 * torch.arange(n_out, dtype=torch.float64) / new)
    edge = int(round(0.01 * new))
    return x, want, slice(edge, n_out - edge)


def check_forward(fn, orig, new, x, label):
    """fn(x2d) -> y; asserts the derived bound first on the reference's own fp32 arithmetic, then on the kernel."""
    want = resample(x, orig, new, torch.float64)
    bound = forward_bound(orig, new, float(x.abs().max()))
    ref32 = float((resample(x, orig, new, torch.float32).double() - want).abs().max())
    assert ref32 <= bound, f"{label}: the fp32 conv1d of the restatement misses its own bound ({ref32:.3e} > {bound:.3e})"
    got = fn(x)
    assert got.shape == want.shape
    err = float((got.double().cpu() - want).abs().max())
    print(f"\n[{label}] |y - y_f64| = {err:.3e} (fp32 conv1d {ref32:.3e}, bound {bound:.3e})")
    assert err <= bound, label
    return err
