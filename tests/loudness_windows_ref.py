"""Float64 restatement of the windowed loudness (``mst_loudness_windows``, include/diffmst_hip.h): the whole signal is K-weighted ONCE
(``loudness_ref.k_weighting``), the energies of its complete gating blocks are taken with ``loudness_ref.block_bounds``, and every
window of ``W`` blocks at a hop of ``H`` blocks is gated on its own.  Also the calls through a bound library that the simulator and the
GPU tests share.

TEST INFRASTRUCTURE: numpy only (and torch for the calls).
"""
import ctypes

import numpy as np
import torch

import loudness_ref as R


def num_complete_blocks(n, rate):
    """Blocks j with bound[j + 4] <= n, by looking at the boundaries (the kernels' host side counts floor((n - 0.4 rate) / (0.1 rate)) + 1)."""
    nb = 0
    while R.block_bounds(nb, rate)[1] <= n:
        nb += 1
    return nb


def num_windows(nb, W, H):
    return (nb - W) // H + 1


def block_energies(x, rate):
    """x (channels, n) float -> z (channels, NB) float64: mean square of the K-weighted signal over every complete block."""
    y = np.asarray(x, dtype=np.float64).copy()
    for b, a in R.k_weighting(rate):
        for c in range(y.shape[0]):
            y[c] = R._lfilter(b, a, y[c])
    nb = num_complete_blocks(y.shape[1], rate)
    z = np.zeros((y.shape[0], nb))
    for j in range(nb):
        lo, hi = R.block_bounds(j, rate)
        z[:, j] = np.sum(np.square(y[:, lo:hi]), axis=1) / (R.T_G * rate)
    return z


def gate(z):
    """BS.1770 gating over the blocks of z (channels, K) -> (lufs, block loudness l (K), absolute set, final set)."""
    G = np.array(R.GAINS[:z.shape[0]])
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(np.sum(G[:, None] * z, axis=0))
        a = [j for j in range(z.shape[1]) if l[j] >= R.ABS_GATE]
        gamma_r = -0.691 + 10.0 * np.log10(np.sum(G * (np.mean(z[:, a], axis=1) if a else 0.0))) - 10.0
        f = [j for j in range(z.shape[1]) if l[j] > gamma_r and l[j] > R.ABS_GATE]
        lufs = float(-0.691 + 10.0 * np.log10(np.sum(G * (np.mean(z[:, f], axis=1) if f else 0.0))))
    return lufs, l, a, f


def windowed_loudness(x, rate, W, H):
    """x (channels, n) -> (lufs (NW,) float64 with -inf for an empty final set, [(l, absolute set, final set)] per window)."""
    z = block_energies(x, rate)
    out, sets = [], []
    for w in range(num_windows(z.shape[1], W, H)):
        lufs, l, a, f = gate(z[:, w * H:w * H + W])
        out.append(lufs)
        sets.append((l, a, f))
    return np.array(out), sets


def window_margins(l):
    """(distance of the nearest block to the relative gate, to the absolute gate) of one window, from its block loudness alone.
    A window with no block above the absolute gate has no relative gate to sit on."""
    fin = l[np.isfinite(l)]
    m_abs = float(np.min(np.abs(fin - R.ABS_GATE))) if len(fin) else np.inf
    a, gamma_r, _ = R.gate_sets(l)
    m_rel = float(np.min(np.abs(fin - gamma_r))) if a and len(fin) else np.inf
    return m_rel, m_abs


def kernel_gate_sets(l_blocks, W, H, w):
    """Gate sets of window w recomputed from the kernel's own fp32 block loudness (``mst_loudness_integrated``'s block_loudness)."""
    a, _, f = R.gate_sets(l_blocks[w * H:w * H + W])
    return a, f


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def count_windows(L, n, rate, W, H):
    """``mst_loudness_num_windows`` -> NW, or 0 when it refuses (it reports a status and writes the count through a host pointer)."""
    from mst import _cabi

    out = ctypes.c_int32(-7)
    try:
        L.mst_loudness_num_windows(n, rate, W, H, ctypes.byref(out))
    except _cabi.AbiError:
        assert out.value == 0
        return 0
    assert out.value > 0
    return out.value


def call_windows(L, x, rate, tables, W, H, want_lufs=True, fill=float("nan")):
    """x fp32 tensor (rows, channels, n), any row / channel stride, on the device of `tables` -> (window_lufs (rows, NW), lufs (rows) or
    None) as tensors.  The workspace is filled with `fill`: the kernels must not rely on a cleared one."""
    rows, chs, n = x.shape
    assert x.stride(2) == 1
    nw = count_windows(L, n, rate, W, H)
    nbytes = L.mst_loudness_windows_workspace_bytes(rows, chs, n, rate, W, H)
    assert nw > 0 and nbytes > 0
    ws = torch.full((nbytes // 8 + 1,), fill, dtype=torch.float64, device=x.device)
    out = torch.full((rows, nw), float("nan"), device=x.device)
    lufs = torch.full((rows,), float("nan"), device=x.device) if want_lufs else None
    L.mst_loudness_windows(x, rows, chs, n, x.stride(0), x.stride(1), rate, tables, W, H, out, lufs, ws, nbytes, None)
    return out, lufs
