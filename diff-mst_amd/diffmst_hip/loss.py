"""``diffmst_hip.loss`` (alias ``mst.loss``) - the losses on the hot path, MI355X-native.

* ``MultiResolutionSTFTLoss`` - drop-in for ``auraloss.freq.MultiResolutionSTFTLoss`` as the reference
  configures it (configs/models/naive.yaml:54-68; evaluation instance mst/system.py:61-69): same
  constructor keywords for the supported subset, called as ``loss(pred, target)`` -> scalar tensor.
  The windowed real-FFT spectrograms, magnitude / log / norm reductions and their adjoints run in
  ``diff-mst_amd/csrc/mst_stft.hip``; no spectrogram is ever materialised.
* ``AudioFeatureLoss`` - reference mst/loss.py:198-260 (see below).
"""
from __future__ import annotations

import ctypes
from typing import List

import torch
from torch.autograd.function import once_differentiable

from . import _cabi, _hip

_TABLE_CACHE = {}


def _mrstft_desc(rows, n, resolutions, w_sc, w_log_mag, w_lin_mag, sc_per_example, eps):
    d = _cabi.MrstftDesc()
    d.rows, d.n_samples, d.n_res = int(rows), int(n), len(resolutions)
    for i, (nf, hop, win) in enumerate(resolutions):
        d.fft_size[i], d.hop_size[i], d.win_length[i] = int(nf), int(hop), int(win)
    d.w_sc, d.w_log_mag, d.w_lin_mag = float(w_sc), float(w_log_mag), float(w_lin_mag)
    d.sc_per_example, d.eps = int(bool(sc_per_example)), float(eps)
    return d


def _tables(desc, resolutions, device):
    """Twiddle + window tables: depend only on (fft_size, win_length); built once per device."""
    lib = _hip.lib()
    key = (str(device), tuple((r[0], r[2]) for r in resolutions))
    return _hip.device_tables(_TABLE_CACHE, key, device, lib.mst_mrstft_tables_bytes, lib.mst_mrstft_init_tables, desc,
                              unsupported="unsupported STFT configuration (fft sizes must be powers of two in 128..8192, "
                                          "win_length <= fft_size, n_samples > fft_size/2)")


class _MrstftFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, cfg, want_grad=True):
        _hip.require_cuda(pred, target)
        if ctx.needs_input_grad[1]:
            # auraloss differentiates w.r.t. both arguments; no in-repo caller of the reference asks for the target's gradient
            # (mst/system.py:331-338: the target is the detached reference mix) and the adjoint kernels do not form it
            raise NotImplementedError("MultiResolutionSTFTLoss (MI355X build): the target's gradient is not implemented; detach the target")
        # the backward is wanted when the prediction requires grad AND grad mode is on at the call (forward() itself runs with grad
        # mode off, so the module hands the caller's mode over): under torch.no_grad() the value-only forward keeps no spectra
        want_grad = bool(want_grad) and ctx.needs_input_grad[0]
        ctx.saved = False
        lib = _hip.lib()
        n = pred.shape[-1]
        x = pred.float().reshape(-1, n).contiguous()
        y = target.float().reshape(-1, n).contiguous()
        if x.shape != y.shape:
            raise ValueError(f"input {tuple(pred.shape)} and target {tuple(target.shape)} differ")
        dev = x.device
        desc = _mrstft_desc(x.shape[0], n, cfg["resolutions"], cfg["w_sc"], cfg["w_log_mag"], cfg["w_lin_mag"],
                            cfg["sc_per_example"], cfg["eps"])
        tables = _tables(desc, cfg["resolutions"], dev)
        nbytes = lib.mst_mrstft_workspace_bytes(desc)
        if nbytes == 0:
            raise ValueError("unsupported STFT configuration for this input length")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        group = cfg.get("sync_group")
        if group is not None and not cfg["sc_per_example"]:
            # batch rows sharded over ranks + batch-global spectral convergence: the two squared norms are summed over the
            # ranks before the division (include/diffmst_hip.h, mst_mrstft_forward_partial / _finish)
            import torch.distributed as dist

            totals = torch.empty(len(cfg["resolutions"]) * 4, dtype=torch.float64, device=dev)
            with _hip.launch_on(dev) as st:
                lib.mst_mrstft_forward_partial(desc, x, y, tables, totals, ws, nbytes, st)
            grp = None if group is True else group
            if dist.get_backend(grp) == "gloo":  # CPU collectives: a 96-byte round trip through the host
                host = totals.cpu()
                dist.all_reduce(host, group=grp)
                totals.copy_(host)
            else:
                dist.all_reduce(totals, group=grp)
            with _hip.launch_on(dev) as st:
                lib.mst_mrstft_forward_finish(desc, totals, dist.get_world_size(grp), loss, ws, nbytes, st)
        else:
            # no gradient asked for (torch.no_grad(), a detached prediction): the value only - the forward then keeps no spectra
            fwd = lib.mst_mrstft_forward if want_grad else lib.mst_mrstft_forward_eval
            with _hip.launch_on(dev) as st:
                fwd(desc, x, y, tables, loss, ws, nbytes, st)
        if want_grad:
            ctx.desc, ctx.nbytes, ctx.shape = desc, nbytes, pred.shape
            ctx.save_for_backward(x, y, tables, ws)
            ctx.saved = True
        return loss.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.saved:  # nothing was kept (value-only forward): there is no gradient to hand back
            return None, None, None, None
        x, y, tables, ws = ctx.saved_tensors
        lib = _hip.lib()
        dev = x.device
        g = grad_loss.float().reshape(1).contiguous()
        gx = torch.empty_like(x)
        with _hip.launch_on(dev) as st:
            lib.mst_mrstft_backward(ctx.desc, x, y, tables, g, gx, ws, ctx.nbytes, st)
        return gx.view(ctx.shape), None, None, None


def _mrstft_check_items(items, rows):
    """``items`` groups of consecutive rows of the leading dimension: a positive whole number that divides it -> that number."""
    if isinstance(items, bool) or int(items) != items or int(items) < 1:
        raise ValueError(f"items must be a positive whole number, got {items!r}")
    if rows % int(items):
        raise ValueError(f"the input's leading dimension is {rows}, which items={items} does not divide (rows are item-major)")
    return int(items)


class _MrstftItemsFunction(torch.autograd.Function):
    """``_MrstftFunction`` with every group of ``shape[0] / items`` leading entries a loss of its own: an ``(items,)`` output, a
    cotangent per item (``mst_mrstft_forward_items`` / ``_backward_items``)."""

    @staticmethod
    def forward(ctx, pred, target, cfg, items, want_grad=True):
        _hip.require_cuda(pred, target)
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("MultiResolutionSTFTLoss (MI355X build): the target's gradient is not implemented; detach the target")
        want_grad = bool(want_grad) and ctx.needs_input_grad[0]
        ctx.saved = False
        lib = _hip.lib()
        n = pred.shape[-1]
        x = pred.float().reshape(-1, n).contiguous()
        y = target.float().reshape(-1, n).contiguous()
        if x.shape != y.shape:
            raise ValueError(f"input {tuple(pred.shape)} and target {tuple(target.shape)} differ")
        dev = x.device
        desc = _mrstft_desc(x.shape[0], n, cfg["resolutions"], cfg["w_sc"], cfg["w_log_mag"], cfg["w_lin_mag"],
                            cfg["sc_per_example"], cfg["eps"])
        tables = _tables(desc, cfg["resolutions"], dev)
        nbytes = lib.mst_mrstft_workspace_bytes(desc)
        if nbytes == 0:
            raise ValueError("unsupported STFT configuration for this input length")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        losses = torch.empty(items, dtype=torch.float32, device=dev)
        # no gradient asked for (torch.no_grad(), a detached prediction): the values only - the forward then keeps no spectra
        fwd = lib.mst_mrstft_forward_items if want_grad else lib.mst_mrstft_forward_items_eval
        with _hip.launch_on(dev) as st:
            fwd(desc, items, x, y, tables, losses, ws, nbytes, st)
        if want_grad:
            ctx.desc, ctx.nbytes, ctx.shape, ctx.items = desc, nbytes, pred.shape, items
            ctx.save_for_backward(x, y, tables, ws)
            ctx.saved = True
        return losses

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_losses):
        if not ctx.saved:  # nothing was kept (value-only forward): there is no gradient to hand back
            return None, None, None, None, None
        x, y, tables, ws = ctx.saved_tensors
        lib = _hip.lib()
        g = grad_losses.float().reshape(ctx.items).contiguous()
        gx = torch.empty_like(x)
        with _hip.launch_on(x.device) as st:
            lib.mst_mrstft_backward_items(ctx.desc, ctx.items, x, y, tables, g, gx, ws, ctx.nbytes, st)
        return gx.view(ctx.shape), None, None, None, None


class MultiResolutionSTFTLoss(torch.nn.Module):
    """auraloss-compatible multi-resolution STFT loss (spectral convergence + log / linear magnitude L1).

    ``sc_per_example`` selects auraloss 0.4.0's per-example spectral-convergence ratio (default) or the
    batch-global ratio of older releases (SURVEY A.7 - the pinned package is not available to verify).
    Phase loss, mel / chroma scaling, perceptual weighting and scale invariance are not part of the
    reference's configuration and raise ``NotImplementedError``.

    ``sync_group`` (``True`` = the default process group, or a ``torch.distributed`` group; only matters with
    ``sc_per_example=False``): the batch is sharded over the ranks of the group and the batch-global ratio is formed from
    norms summed over all ranks, so that the mean of the rank losses - and rank-averaged gradients - equal the
    single-process values over the global batch.  Every other term is a mean over examples and needs no exchange.
    """

    def __init__(
        self,
        fft_sizes: List[int] = [1024, 2048, 512],
        hop_sizes: List[int] = [120, 240, 50],
        win_lengths: List[int] = [600, 1200, 240],
        window: str = "hann_window",
        w_sc: float = 1.0,
        w_log_mag: float = 1.0,
        w_lin_mag: float = 0.0,
        w_phs: float = 0.0,
        sample_rate: float = None,
        scale: str = None,
        n_bins: int = None,
        perceptual_weighting: bool = False,
        scale_invariance: bool = False,
        eps: float = 1e-8,
        sc_per_example: bool = True,
        sync_group=None,
        **kwargs,
    ):
        super().__init__()
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        if window != "hann_window":
            raise NotImplementedError("only the (default) periodic Hann window is built")
        if w_phs or scale is not None or perceptual_weighting or scale_invariance:
            raise NotImplementedError("phase loss / mel-chroma scaling / perceptual weighting / scale invariance "
                                      "are outside the reference's configuration of this loss")
        self.fft_sizes, self.hop_sizes, self.win_lengths = list(fft_sizes), list(hop_sizes), list(win_lengths)
        self.cfg = dict(
            resolutions=tuple(zip(self.fft_sizes, self.hop_sizes, self.win_lengths)),
            w_sc=w_sc, w_log_mag=w_log_mag, w_lin_mag=w_lin_mag, sc_per_example=sc_per_example, eps=eps,
            sync_group=sync_group,
        )

    # sample against sample: no profile of a reference stands in for it.  mst.online's sectioned fits read this and hand the
    # reference itself to ``pooled``, cut like the tracks
    paired = True

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return _MrstftFunction.apply(x, y, self.cfg, torch.is_grad_enabled())

    def per_item(self, input: torch.Tensor, target: torch.Tensor, items: int = None) -> torch.Tensor:
        """The loss of every item on its own: an ``(items,)`` float32 device tensor, element ``b`` what ``forward`` returns for item
        ``b``'s part of ``input`` and ``target`` alone, differentiable in ``input``; a cotangent on element ``b`` reaches item ``b``
        only, and no gradient carries a ``1 / items`` (``AudioFeatureLoss.per_item``'s convention: under the batch mean Adam's ``eps``
        makes that factor visible).  ``input`` and ``target`` have ``forward``'s shapes, ``(bs, chs, n)``; ``items`` defaults to
        ``bs`` and must divide it: item ``b`` is ``input[b * bs / items:(b + 1) * bs / items]``, all channels - with
        ``sc_per_example=False`` the ratio is taken over the item's rows.  One pass over the batch (``mst_mrstft_forward_items``):
        ``forward``'s transform launches, then a reduction that folds in a fixed order, so equal inputs give equal bits and
        ``items=1`` gives ``forward``'s.  For per-song validation figures and for a batch of independent fits
        (``mst.online.optimize_batch``).

        Under ``torch.no_grad()`` or with a detached ``input`` only the values are computed and nothing is kept.  The target's
        gradient is refused, as in ``forward``; so is ``sync_group``: a ratio over the rows of every rank has no per-item meaning."""
        if self.cfg.get("sync_group") is not None:
            raise ValueError("MultiResolutionSTFTLoss.per_item / pooled: not with sync_group - a ratio formed over the rows of every "
                             "rank has no per-item meaning; build the loss without it")
        if not isinstance(input, torch.Tensor) or not isinstance(target, torch.Tensor):
            raise TypeError("MultiResolutionSTFTLoss.per_item takes two tensors")
        if target.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("MultiResolutionSTFTLoss (MI355X build): the target's gradient is not implemented; detach the target")
        if input.dim() < 2:
            raise ValueError(f"per_item takes an input of shape (bs, ..., n), got {tuple(input.shape)}")
        if input.shape != target.shape:
            raise ValueError(f"input {tuple(input.shape)} and target {tuple(target.shape)} differ")
        items = _mrstft_check_items(input.shape[0] if items is None else items, input.shape[0])
        return _MrstftItemsFunction.apply(input, target, self.cfg, items, torch.is_grad_enabled())

    def pooled(self, input: torch.Tensor, target: torch.Tensor, items: int = 1) -> torch.Tensor:
        """``per_item`` with ``items`` defaulting to 1: the ``S`` sections of one fit, ``input (S, 2, n)``, are ONE item of ``2 S`` rows
        and the result is ``(1,)``.  For this loss every term is a mean over rows (or a ratio of sums over them), so pooling the
        sections is the loss of the sections taken as one batch.  ``items=B``: ``input`` is ``(B * S, 2, n)``, item-major, and the
        result ``(B,)`` (``mst.online.optimize_sections`` / ``optimize_sections_batch``).  ``target`` is cut like ``input``."""
        return self.per_item(input, target, items)


# ------------------------------------------------------------------------------------------------
# AudioFeatureLoss
# ------------------------------------------------------------------------------------------------
AF_KEYS = ("mix-rms", "mix-crest_factor", "mix-stereo_width", "mix-stereo_imbalance", "mix-barkspectrum")
_AF_CACHE = {}   # engine tables per (device, sample rate)
_AF_FBANKS = {}  # the Bark filterbank beside them, same key


def _af_constants(device, sample_rate):
    """(twiddle/window tables, Bark filterbank) on `device`; built once."""
    lib = _hip.lib()
    key = (str(device), int(sample_rate))
    tables = _hip.device_tables(_AF_CACHE, key, device, lib.mst_afloss_tables_bytes, lib.mst_afloss_init_tables)
    fb = _AF_FBANKS.get(key)
    if fb is None:
        from .filter import barkscale_fbanks

        fb = barkscale_fbanks(16385, 20.0, 20000.0, 24, sample_rate).contiguous().to(device)  # reference mst/loss.py:88
        _AF_FBANKS[key] = fb
    return tables, fb


class _AudioFeatureFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weights, sample_rate):
        _hip.require_cuda(pred, target)
        lib = _hip.lib()
        if pred.dim() != 3 or pred.shape[1] != 2 or pred.shape != target.shape:
            raise ValueError("AudioFeatureLoss expects (bs, 2, seq_len) input and target of equal shape")
        x = pred.float().contiguous()
        y = target.float().contiguous()
        bs, _, n = x.shape
        dev = x.device
        tables, fb = _af_constants(dev, sample_rate)
        nbytes = lib.mst_afloss_workspace_bytes(bs, n)
        if nbytes == 0:
            raise ValueError("AudioFeatureLoss needs seq_len > 16384 (reflect padding of the 32768-point Bark STFT)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        losses = torch.empty(5, dtype=torch.float32, device=dev)
        w = (ctypes.c_float * 5)(*[float(v) for v in weights])
        with _hip.launch_on(dev) as st:
            lib.mst_afloss_forward(x, y, bs, n, w, tables, fb, losses, ws, nbytes, st)
        ctx.meta = (bs, n, w, nbytes, pred.shape)
        ctx.save_for_backward(x, y, tables, fb, ws)
        # five 0-dim outputs (views of one buffer) instead of one (5,) tensor the caller would index: indexing costs
        # ~3 tiny kernels per key in forward + backward, 5 x that is more than the closed-form features themselves
        return tuple(losses.unbind(0))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_each):
        x, y, tables, fb, ws = ctx.saved_tensors
        bs, n, w, nbytes, shape = ctx.meta
        lib = _hip.lib()
        dev = x.device
        g = torch.stack([gi.float().reshape(()) for gi in grad_each]).contiguous()
        gx = torch.empty_like(x)
        with _hip.launch_on(dev) as st:
            lib.mst_afloss_backward(x, y, bs, n, w, tables, fb, g, gx, ws, nbytes, st)
        return gx.view(shape), None, None, None


class AudioFeatureProfile:
    """The five features of a stereo signal as ``AudioFeatureLoss`` compares them: what is left of a target once it has been analysed.

    ``data`` is a ``(bs, 54)`` float64 device tensor in the layout ``include/diffmst_hip.h`` documents (``MST_AF_PROFILE_DOUBLES``):
    mean L^2, R^2, (L+R)^2, (L-R)^2; max|L|, max|R|; the 24 log Bark band energies of the mid signal, then of the side signal.  None
    of it depends on the length of the signal, so a profile stands in for a target of any length; ``n_samples`` only records what was
    analysed (``None`` for a profile rebuilt from stored ``data``: ``AudioFeatureProfile(data, sample_rate)`` reloads one).

    ``rms``, ``crest_factor``, ``stereo_width``, ``stereo_imbalance`` and ``barkspectrum`` are the values the reference's
    ``compute_rms`` ... ``compute_barkspectrum`` (mst/loss.py:62-195) return for that audio, in its shapes and as float32: a few torch
    operations on the 54 numbers, for reports.  They carry no gradient.
    """

    def __init__(self, data: torch.Tensor, sample_rate: int, n_samples: int = None) -> None:
        if not isinstance(data, torch.Tensor) or data.dim() != 2 or data.shape[1] != _cabi.AF_PROFILE_DOUBLES or data.dtype != torch.float64:
            raise ValueError(f"a profile is a (bs, {_cabi.AF_PROFILE_DOUBLES}) float64 tensor")
        self.data = data.detach().contiguous()
        self.sample_rate = sample_rate
        self.n_samples = None if n_samples is None else int(n_samples)

    @property
    def batch_size(self) -> int:
        return self.data.shape[0]

    def to(self, device) -> "AudioFeatureProfile":
        return AudioFeatureProfile(self.data.to(device), self.sample_rate, self.n_samples)

    @property
    def rms(self) -> torch.Tensor:  # (bs, 2)
        return self.data[:, 0:2].clamp(min=1e-8).sqrt().float()

    @property
    def crest_factor(self) -> torch.Tensor:  # (bs, 2), dB
        rms = self.data[:, 0:2].clamp(min=1e-8).sqrt()
        return (20.0 * torch.log10((self.data[:, 4:6] / rms.clamp(min=1e-8)).clamp(min=1e-8))).float()

    @property
    def stereo_width(self) -> torch.Tensor:  # (bs,)
        return (self.data[:, 3] / self.data[:, 2].clamp(min=1e-8)).float()

    @property
    def stereo_imbalance(self) -> torch.Tensor:  # (bs,)
        el, er = self.data[:, 0], self.data[:, 1]
        return ((er - el) / (er + el).clamp(min=1e-8)).float()

    @property
    def barkspectrum(self) -> torch.Tensor:  # (bs, 24, 2): [..., 0] mid, [..., 1] side
        return torch.stack((self.data[:, 6:30], self.data[:, 30:54]), dim=-1).float()


def _af_check_input(x, what):
    if x.dim() != 3 or x.shape[1] != 2:
        raise ValueError(f"AudioFeatureLoss expects a (bs, 2, seq_len) {what}, got {tuple(x.shape)}")


def _af_check_items(items, rows, what):
    """``items`` groups of consecutive rows: a positive whole number that divides the row count -> that number."""
    if isinstance(items, bool) or int(items) != items or int(items) < 1:
        raise ValueError(f"items must be a positive whole number, got {items!r}")
    if rows % int(items):
        raise ValueError(f"the {what} has {rows} rows, which items={items} does not divide (rows are item-major: items * sections)")
    return int(items)


class _AudioFeatureProfileFunction(torch.autograd.Function):
    """The loss of ``pred`` against a profile: the prediction's half of ``_AudioFeatureFunction``'s work."""

    @staticmethod
    def forward(ctx, pred, profile, weights, sample_rate):
        lib = _hip.lib()
        x = pred.float().contiguous()
        bs, _, n = x.shape
        dev = x.device
        tables, fb = _af_constants(dev, sample_rate)
        nbytes = lib.mst_afloss_profile_workspace_bytes(bs, n)
        if nbytes == 0:
            raise ValueError("AudioFeatureLoss needs seq_len > 16384 (reflect padding of the 32768-point Bark STFT)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        losses = torch.empty(5, dtype=torch.float32, device=dev)
        w = (ctypes.c_float * 5)(*[float(v) for v in weights])
        with _hip.launch_on(dev) as st:
            lib.mst_afloss_forward_profile(x, profile, bs, n, w, tables, fb, losses, ws, nbytes, st)
        ctx.meta = (bs, n, w, nbytes, pred.shape)
        ctx.save_for_backward(x, profile, tables, fb, ws)
        return tuple(losses.unbind(0))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_each):
        x, profile, tables, fb, ws = ctx.saved_tensors
        bs, n, w, nbytes, shape = ctx.meta
        lib = _hip.lib()
        dev = x.device
        g = torch.stack([gi.float().reshape(()) for gi in grad_each]).contiguous()
        gx = torch.empty_like(x)
        with _hip.launch_on(dev) as st:
            lib.mst_afloss_backward_profile(x, profile, bs, n, w, tables, fb, g, gx, ws, nbytes, st)
        return gx.view(shape), None, None, None


class _AudioFeatureItemsFunction(torch.autograd.Function):
    """``_AudioFeatureProfileFunction`` with every batch item a loss of its own: five ``(bs,)`` outputs, a cotangent per item."""

    @staticmethod
    def forward(ctx, pred, profile, weights, sample_rate):
        lib = _hip.lib()
        x = pred.float().contiguous()
        bs, _, n = x.shape
        dev = x.device
        tables, fb = _af_constants(dev, sample_rate)
        nbytes = lib.mst_afloss_profile_workspace_bytes(bs, n)
        if nbytes == 0:
            raise ValueError("AudioFeatureLoss needs seq_len > 16384 (reflect padding of the 32768-point Bark STFT)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        losses = torch.empty(bs, 5, dtype=torch.float32, device=dev)
        w = (ctypes.c_float * 5)(*[float(v) for v in weights])
        with _hip.launch_on(dev) as st:
            lib.mst_afloss_forward_profile_items(x, profile, bs, n, w, tables, fb, losses, ws, nbytes, st)
        ctx.meta = (bs, n, w, nbytes, pred.shape)
        ctx.save_for_backward(x, profile, tables, fb, ws)
        return tuple(losses.unbind(1))  # five (bs,) views of one buffer

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_each):
        x, profile, tables, fb, ws = ctx.saved_tensors
        bs, n, w, nbytes, shape = ctx.meta
        lib = _hip.lib()
        dev = x.device
        g = torch.stack([gi.float().reshape(bs) for gi in grad_each], dim=1).contiguous()  # (bs, 5)
        gx = torch.empty_like(x)
        with _hip.launch_on(dev) as st:
            lib.mst_afloss_backward_profile_items(x, profile, bs, n, w, tables, fb, g, gx, ws, nbytes, st)
        return gx.view(shape), None, None, None


class _AudioFeaturePooledFunction(torch.autograd.Function):
    """The loss of the rows of ``pred`` TAKEN TOGETHER, ``items`` groups of consecutive rows against a profile row each: five
    ``(items,)`` outputs, a cotangent row per item."""

    @staticmethod
    def forward(ctx, pred, profile, weights, sample_rate, items=1):
        lib = _hip.lib()
        x = pred.float().contiguous()
        bs, _, n = x.shape
        sections = bs // items
        dev = x.device
        tables, fb = _af_constants(dev, sample_rate)
        nbytes = lib.mst_afloss_profile_workspace_bytes(bs, n)
        if nbytes == 0:
            raise ValueError("AudioFeatureLoss needs seq_len > 16384 (reflect padding of the 32768-point Bark STFT)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        losses = torch.empty(items, 5, dtype=torch.float32, device=dev)
        w = (ctypes.c_float * 5)(*[float(v) for v in weights])
        with _hip.launch_on(dev) as st:
            lib.mst_afloss_forward_profile_pooled(x, profile, items, sections, n, w, tables, fb, losses, ws, nbytes, st)
        ctx.meta = (items, sections, n, w, nbytes, pred.shape)
        ctx.save_for_backward(x, profile, tables, fb, ws)
        return tuple(losses.unbind(1))  # five (items,) views of one buffer

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_each):
        x, profile, tables, fb, ws = ctx.saved_tensors
        items, sections, n, w, nbytes, shape = ctx.meta
        lib = _hip.lib()
        dev = x.device
        g = torch.stack([gi.float().reshape(items) for gi in grad_each], dim=1).contiguous()  # (items, 5)
        gx = torch.empty_like(x)
        with _hip.launch_on(dev) as st:
            lib.mst_afloss_backward_profile_pooled(x, profile, items, sections, n, w, tables, fb, g, gx, ws, nbytes, st)
        return gx.view(shape), None, None, None, None


class AudioFeatureLoss(torch.nn.Module):
    """Drop-in for reference ``mst.loss.AudioFeatureLoss`` (:198-260).

    ``forward(input, target)`` returns ``{key: weight * mse(feature(input), feature(target))}`` with the
    reference's five keys (``System`` sums ``val.mean()`` over them, mst/system.py:334-336).  All five
    features and their gradients are computed by the kernels of ``csrc/mst_af.hip`` in one pass.

    The features are aggregates over time, so - as in the reference - the target need not have the input's length: a ``(bs, 2, m)``
    target with ``m != seq_len`` is analysed into an ``AudioFeatureProfile`` and the loss runs against that; ``profile(x)`` returns
    the profile itself, to be passed as ``target`` wherever one target meets many inputs (``mst.online.optimize``): the target's
    transforms then run once instead of in every call.  A target of the input's shape takes the paired kernels, as it always has.
    """

    def __init__(self, weights: List[float], sample_rate: int, stem_separation: bool = False, use_clap: bool = False) -> None:
        super().__init__()
        self.weights = weights
        self.sample_rate = sample_rate
        self.stem_separation = stem_separation
        self.sources_list = ["mix"]
        self.source_weights = [1.0]
        self.use_clap = use_clap
        self.transform_names = ["rms", "crest_factor", "stereo_width", "stereo_imbalance", "barkspectrum"]
        assert len(self.transform_names) == len(weights)

    Profile = AudioFeatureProfile  # reachable wherever this class is: ``mst.loss.AudioFeatureLoss.Profile`` after ``install()``

    @torch.no_grad()
    def profile(self, x: torch.Tensor, pool: bool = False, items: int = 1) -> AudioFeatureProfile:
        """Analyse ``x (bs, 2, n)``, ``n > 16384``, on its device -> ``AudioFeatureProfile``.  No gradient reaches ``x``: the target
        side of this loss never receives one.

        ``pool=True``: the rows of ``x`` are sections of ONE signal and the result is one profile of batch size 1, pooled over them as
        ``pooled`` pools its input (``include/diffmst_hip.h``, ``mst_af_profile_pooled``): rms, crest factor, width and imbalance of the
        concatenation, the mean magnitude spectrum over all frames of all sections.  For a reference given as sections.  With
        ``items=B`` as well, ``x`` is ``(B * R, 2, n)``, item-major, and the result has batch size ``B``: every item pooled over its
        own ``R`` rows."""
        _hip.require_cuda(x)
        _af_check_input(x, "signal")
        if not pool and items != 1:
            raise ValueError("items needs pool=True: without pooling every row of x is a profile row of its own")
        items = _af_check_items(items, x.shape[0], "signal")
        lib = _hip.lib()
        x = x.detach().float().contiguous()
        bs, _, n = x.shape
        dev = x.device
        nbytes = lib.mst_af_profile_workspace_bytes(bs, n)
        if nbytes == 0:
            raise ValueError("AudioFeatureLoss needs seq_len > 16384 (reflect padding of the 32768-point Bark STFT)")
        tables, fb = _af_constants(dev, self.sample_rate)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        data = torch.empty(items if pool else bs, _cabi.AF_PROFILE_DOUBLES, dtype=torch.float64, device=dev)
        with _hip.launch_on(dev) as st:
            if pool:
                lib.mst_af_profile_pooled(x, items, bs // items, n, tables, fb, data, ws, nbytes, st)
            else:
                lib.mst_af_profile(x, bs, n, tables, fb, data, ws, nbytes, st)
        return AudioFeatureProfile(data, self.sample_rate, bs // items * n if pool else n)

    def pooled(self, input: torch.Tensor, target, items: int = 1):
        """The five terms of the rows of ``input (S, 2, n)`` TAKEN TOGETHER - S sections of one mix as one signal:
        ``{key: (1,) float32 device tensor}``, differentiable in ``input``.  All five features are aggregates over time, so the features
        of several sections are formed from the sections' sums, peaks and mean magnitudes before the nonlinear maps
        (``mst_afloss_forward_profile_pooled``): rms, crest factor, width and imbalance are those of ``torch.cat(sections, dim=-1)``,
        the Bark spectrum that of the mean magnitude over all frames of all sections.  This is not the mean of ``per_item``'s rows: the mean of
        S crest factors is not the crest factor of the whole.  ``S = 1`` is ``per_item`` at batch 1, bit for bit.

        ``target`` is an ``AudioFeatureProfile`` of batch size 1 or a ``(1, 2, m)`` tensor of any length ``m > 16384``, which is
        profiled on the way.  Errors as ``per_item``'s.

        ``items=B`` pools ``B`` groups at once: ``input`` is ``(B * S, 2, n)``, item-major (row ``b * S + s`` is section ``s`` of item
        ``b``), the terms are ``(B,)`` tensors, a cotangent on element ``b`` reaches item ``b``'s rows only, and ``target`` is a profile
        of batch size ``B`` or 1 (one reference for every item) or a ``(B, 2, m)`` tensor.  A row count that ``items`` does not divide
        raises ``ValueError``.  For a batch of sectioned fits (``mst.online.optimize_sections_batch``)."""
        is_profile = isinstance(target, AudioFeatureProfile)
        if not is_profile and not isinstance(target, torch.Tensor):
            raise TypeError(f"AudioFeatureLoss takes a tensor or an AudioFeatureProfile as target, got {type(target).__name__}")
        _hip.require_cuda(input, target.data if is_profile else target)
        _af_check_input(input, "input")
        if is_profile:
            if target.sample_rate != self.sample_rate:
                raise ValueError(f"the profile was taken at {target.sample_rate} Hz, this loss runs at {self.sample_rate} Hz")
        else:
            _af_check_input(target, "target")
        items = _af_check_items(items, input.shape[0], "input")
        have = target.batch_size if is_profile else target.shape[0]
        if have != items and not (is_profile and have == 1):
            if items == 1:
                raise ValueError(f"the sections of the input are pooled into one row, the target has batch size {have}")
            raise ValueError(f"the sections of the input are pooled into {items} rows, the target has batch size {have}")
        if not is_profile:
            target = self.profile(target)
        _hip.require_same_device(input.device, target.data)
        data = target.data if have == items else target.data.expand(items, -1).contiguous()
        losses = _AudioFeaturePooledFunction.apply(input, data, tuple(self.weights), self.sample_rate, items)
        return dict(zip(AF_KEYS, losses))

    def per_item(self, input: torch.Tensor, target):
        """The five terms of every batch item on its own: ``{key: (bs,) float32 device tensor}``, row ``b`` what ``forward`` returns for
        ``input[b:b + 1]`` alone (the batch mean of each key is ``forward``'s value), differentiable in ``input``; a cotangent on
        element ``b`` reaches ``input[b]`` only.  For a batch of independent fits (``mst.online.optimize_batch``): under ``forward``
        every item's gradient carries the factor ``1 / bs``, which Adam's ``eps`` makes visible.

        ``target`` is an ``AudioFeatureProfile`` of batch size ``bs`` or 1 (one reference for every item) or a ``(bs, 2, m)`` tensor of
        any length ``m > 16384``, which is profiled on the way - also when ``m == seq_len``: this route has no paired kernels."""
        is_profile = isinstance(target, AudioFeatureProfile)
        if not is_profile and not isinstance(target, torch.Tensor):
            raise TypeError(f"AudioFeatureLoss takes a tensor or an AudioFeatureProfile as target, got {type(target).__name__}")
        _hip.require_cuda(input, target.data if is_profile else target)
        _af_check_input(input, "input")
        bs = input.shape[0]
        if is_profile:
            if target.sample_rate != self.sample_rate:
                raise ValueError(f"the profile was taken at {target.sample_rate} Hz, this loss runs at {self.sample_rate} Hz")
        else:
            _af_check_input(target, "target")
        have = target.batch_size if is_profile else target.shape[0]
        if have != bs and not (is_profile and have == 1):
            raise ValueError(f"input has batch size {bs}, the target {have}")
        if not is_profile:
            target = self.profile(target)
        _hip.require_same_device(input.device, target.data)
        data = target.data if have == bs else target.data.expand(bs, -1).contiguous()
        losses = _AudioFeatureItemsFunction.apply(input, data, tuple(self.weights), self.sample_rate)
        return dict(zip(AF_KEYS, losses))

    def forward(self, input: torch.Tensor, target):
        if isinstance(target, torch.Tensor) and target.shape == input.shape:
            losses = _AudioFeatureFunction.apply(input, target, tuple(self.weights), self.sample_rate)
            return dict(zip(AF_KEYS, losses))
        is_profile = isinstance(target, AudioFeatureProfile)
        if not is_profile and not isinstance(target, torch.Tensor):
            raise TypeError(f"AudioFeatureLoss takes a tensor or an AudioFeatureProfile as target, got {type(target).__name__}")
        _hip.require_cuda(input, target.data if is_profile else target)
        _af_check_input(input, "input")
        if is_profile:
            if target.sample_rate != self.sample_rate:
                raise ValueError(f"the profile was taken at {target.sample_rate} Hz, this loss runs at {self.sample_rate} Hz")
        else:
            _af_check_input(target, "target")
        if (target.batch_size if is_profile else target.shape[0]) != input.shape[0]:
            raise ValueError(f"input has batch size {input.shape[0]}, the target {target.batch_size if is_profile else target.shape[0]}")
        if not is_profile:
            target = self.profile(target)  # another length: the reference takes it (its features are means and maxima over time)
        _hip.require_same_device(input.device, target.data)
        losses = _AudioFeatureProfileFunction.apply(input, target.data, tuple(self.weights), self.sample_rate)
        return dict(zip(AF_KEYS, losses))
