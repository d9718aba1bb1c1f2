"""Float64 restatement of ``pyloudnorm.Meter(rate).integrated_loudness`` (ITU-R BS.1770-4 integrated loudness with
pyloudnorm's defaults: filter class "K-weighting", block size 0.400 s), written from the published source.

PARITY UNPINNED: pyloudnorm is not installed where this project is built and tested, so this file was never run
against it.  What ties it to BS.1770 is the standard's calibration point (997 Hz, 0 dBFS, one channel -> -3.01 LKFS)
and the closed-form level of stationary sines, both asserted in tests/test_loudness_hostsim.py.

TEST INFRASTRUCTURE: numpy only (scipy.signal.lfilter is used when scipy imports, a plain recursion otherwise).
"""
import math

import numpy as np

T_G = 0.4          # gating block, seconds
OVERLAP = 0.75
STEP = 1.0 - OVERLAP
GAINS = (1.0, 1.0, 1.0, 1.41, 1.41)
ABS_GATE = -70.0


def k_weighting(rate):
    """[(b, a)] of the two biquads, float64, normalised by a0 (pyloudnorm IIRfilter 'high_shelf' and 'high_pass')."""
    out = []
    # high shelf: G = 4 dB, Q = 1/sqrt(2), fc = 1500 Hz
    G, Q, fc = 4.0, 1.0 / math.sqrt(2.0), 1500.0
    A = 10.0 ** (G / 40.0)
    w0 = 2.0 * math.pi * (fc / rate)
    alpha = math.sin(w0) / (2.0 * Q)
    c = math.cos(w0)
    b0 = A * ((A + 1) + (A - 1) * c + 2 * math.sqrt(A) * alpha)
    b1 = -2 * A * ((A - 1) + (A + 1) * c)
    b2 = A * ((A + 1) + (A - 1) * c - 2 * math.sqrt(A) * alpha)
    a0 = (A + 1) - (A - 1) * c + 2 * math.sqrt(A) * alpha
    a1 = 2 * ((A - 1) - (A + 1) * c)
    a2 = (A + 1) - (A - 1) * c - 2 * math.sqrt(A) * alpha
    out.append((np.array([b0, b1, b2]) / a0, np.array([a0, a1, a2]) / a0))
    # high pass: Q = 0.5, fc = 38 Hz
    Q, fc = 0.5, 38.0
    w0 = 2.0 * math.pi * (fc / rate)
    alpha = math.sin(w0) / (2.0 * Q)
    c = math.cos(w0)
    b0, b1, b2 = (1 + c) / 2, -(1 + c), (1 + c) / 2
    a0, a1, a2 = 1 + alpha, -2 * c, 1 - alpha
    out.append((np.array([b0, b1, b2]) / a0, np.array([a0, a1, a2]) / a0))
    return out


def response_sq(rate, f):
    """|H(e^{j 2 pi f / rate})|^2 of the K-weighting, from the coefficients."""
    z = np.exp(-1j * 2.0 * math.pi * f / rate)
    h = 1.0
    for b, a in k_weighting(rate):
        h = h * (b[0] + b[1] * z + b[2] * z * z) / (a[0] + a[1] * z + a[2] * z * z)
    return float(abs(h) ** 2)


def _lfilter(b, a, x):
    try:
        from scipy.signal import lfilter
        return lfilter(b, a, x)
    except ImportError:
        y = np.empty_like(x)
        s1 = s2 = 0.0
        b0, b1, b2 = (float(v) for v in b)
        a1, a2 = float(a[1]), float(a[2])
        for i, xi in enumerate(x.tolist()):
            yi = b0 * xi + s1
            s1 = b1 * xi - a1 * yi + s2
            s2 = b2 * xi - a2 * yi
            y[i] = yi
        return y


def num_blocks(n, rate):
    T = n / rate
    return int(np.round((T - T_G) / (T_G * STEP)) + 1)


def block_bounds(j, rate):
    """(lower, upper) sample index of gating block j, evaluated in float64 exactly as pyloudnorm writes it."""
    return int(T_G * (j * STEP) * rate), int(T_G * (j * STEP + 1) * rate)


def integrated_loudness(data, rate, return_blocks=False):
    """data: (n,) or (n, channels) like pyloudnorm.  Returns LUFS (float), optionally also the block loudness l_j."""
    x = np.asarray(data, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n, chs = x.shape
    if chs > 5:
        raise ValueError("Audio must have five channels or less.")
    if n < T_G * rate:
        raise ValueError("Audio must have length greater than the block size.")
    y = x.copy()
    for b, a in k_weighting(rate):
        for c in range(chs):
            y[:, c] = _lfilter(b, a, y[:, c])
    nb = num_blocks(n, rate)
    z = np.zeros((chs, nb))
    for j in range(nb):
        lo, hi = block_bounds(j, rate)
        for c in range(chs):
            z[c, j] = np.sum(np.square(y[lo:hi, c])) / (T_G * rate)
    G = np.array(GAINS[:chs])
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(np.sum(G[:, None] * z, axis=0))
        sel = [j for j in range(nb) if l[j] >= ABS_GATE]
        z_avg = [np.mean(z[c, sel]) if sel else 0.0 for c in range(chs)]
        gamma_r = -0.691 + 10.0 * np.log10(np.sum(G * np.array(z_avg))) - 10.0
        sel = [j for j in range(nb) if l[j] > gamma_r and l[j] > ABS_GATE]
        z_avg = [np.mean(z[c, sel]) if sel else 0.0 for c in range(chs)]
        lufs = float(-0.691 + 10.0 * np.log10(np.sum(G * np.array(z_avg))))
    if return_blocks:
        return lufs, l
    return lufs


def gate_sets(l):
    """Both gates recomputed from block loudness alone: sum_c G_c z[c][j] = 10^((l_j + 0.691) / 10), and the weighted sum of
    the channel means is the mean of that.  Returns (absolute-gated indices, Gamma_r, final indices)."""
    l = np.asarray(l, dtype=np.float64)
    e = 10.0 ** ((l + 0.691) / 10.0)
    a = [j for j in range(len(l)) if l[j] >= ABS_GATE]
    with np.errstate(divide="ignore"):
        gamma_r = -0.691 + 10.0 * np.log10(np.mean(e[a]) if a else 0.0) - 10.0
    f = [j for j in range(len(l)) if l[j] > gamma_r and l[j] > ABS_GATE]
    return a, float(gamma_r), f


def level_step_noise(rows, channels, n, seed, amp=0.1):
    """Test input: seeded white noise (float32, (rows, channels, n)) with level steps - the stretch [0.2 n, 0.55 n) is 30 dB down
    (the relative gate removes its blocks), the stretch [0.55 n, 0.9 n) is at 1e-6 of full level (the absolute gate removes
    them); each holds whole gating blocks from n = 70000 on.  Rows differ in level by 0.7 dB steps."""
    rng = np.random.default_rng(seed)
    x = amp * rng.standard_normal((rows, channels, n))
    x[..., int(0.2 * n):int(0.55 * n)] *= 10.0 ** (-30.0 / 20.0)
    x[..., int(0.55 * n):int(0.9 * n)] *= 1e-6
    x *= (10.0 ** (-0.7 * np.arange(rows) / 20.0))[:, None, None]
    return x.astype(np.float32)


def gate_margins(l):
    """(min_j |l_j - Gamma_r|, min_j |l_j + 70|) of one row: how far the nearest block is from flipping a gate."""
    l = np.asarray(l, dtype=np.float64)
    _, gamma_r, _ = gate_sets(l)
    fin = l[np.isfinite(l)]
    return float(np.min(np.abs(fin - gamma_r))), float(np.min(np.abs(fin - ABS_GATE)))
