"""Per-song mix optimisation on the device: ``optimize()`` and the block renderer of the reference's ``scripts/online.py``.

``optimize`` fits the console's parameters to a reference mix by gradient descent on their logits - no model involved (reference
scripts/online.py:15-123).  The console, the loss and their backwards are the package's kernels; everything the script does around them
per iteration (three sigmoids and their backwards, the sum of the loss dictionary, ``zero_grad``, torch's Adam over three small
tensors, six ``.item()`` host reads) is ONE launch here, ``mst_logit_adam_step`` (csrc/mst_opt.hip, include/diffmst_hip.h): it chains
dL/dp through the sigmoid, applies Adam, writes the next iteration's parameters, appends the loss terms to a history on the device and
keeps the step count there.  The host reads nothing between the first and the last iteration.

PARITY UNPINNED: the script cannot be imported (it imports ``StereoCLAPLoss``, which the reference's ``mst/loss.py`` does not define),
so its loop is restated here and checked against ``torch.optim.Adam`` behind ``torch.sigmoid`` on recorded gradients.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import torch

from . import _cabi, _hip
from .loss import AudioFeatureProfile


def start_point(n_tracks: int, mix_console, init_scale: float = 0.001, generator=None):
    """The script's three host draws (scripts/online.py:39-45), in its order and with its shapes: ``init_scale * torch.randn`` of
    ``(n_tracks, 27)``, ``(1, 25)`` and ``(1, 26)`` from the global generator or ``generator`` - after ``torch.manual_seed(s)`` the
    start point is the script's.  Host tensors."""
    shapes = ((n_tracks, mix_console.num_track_control_params), (1, mix_console.num_fx_bus_control_params),
              (1, mix_console.num_master_bus_control_params))
    return tuple(init_scale * torch.randn(shape, generator=generator) for shape in shapes)


def _segments(logits, params, grads):
    """The segment table of one call: a NULL gradient for a parameter the loss does not reach."""
    seg = (_cabi.LogitAdamSegment * len(logits))()
    for s, (theta, p, g) in zip(seg, zip(logits, params, grads)):
        s.theta, s.p, s.grad_p, s.count = theta.data_ptr(), p.data_ptr(), None if g is None else g.data_ptr(), theta.numel()
    return seg


def _init(logits, params):
    """p <- sigmoid(logits) by the kernel every later p comes from, and a zeroed optimiser state."""
    lib = _hip.lib()
    dev = logits[0].device
    nbytes = lib.mst_logit_adam_state_bytes(sum(t.numel() for t in logits))
    if nbytes == 0:
        raise ValueError("more parameters than the logit-Adam kernel takes (2^20)")
    state = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    with _hip.launch_on(dev) as st:
        lib.mst_logit_adam_init(_segments(logits, params, (None,) * len(logits)), len(logits), state, st)
    return state


class _Run:
    """One optimisation: set-up (the start point goes to the device), ``iterate(n)`` (nothing in it waits for the device) and
    ``finish()`` (the one read of history and status)."""

    def __init__(self, tracks, ref_mix, mix_console, loss_function, init_scale, lr, n_iters, betas, eps, generator, callback, console_flags):
        is_profile = isinstance(ref_mix, AudioFeatureProfile)
        if not is_profile and not isinstance(ref_mix, torch.Tensor):
            raise TypeError(f"ref_mix must be a (2, n_samples) tensor or an AudioFeatureProfile, got {type(ref_mix).__name__}")
        _hip.require_cuda(tracks, ref_mix.data if is_profile else ref_mix)
        if tracks.dim() != 2:
            raise ValueError(f"tracks must be (n_tracks, n_samples), got {tuple(tracks.shape)} (one song per call: no batch dimension)")
        if is_profile:
            if ref_mix.batch_size != 1:
                raise ValueError(f"a profile given as ref_mix must have batch size 1, got {ref_mix.batch_size}")
        elif ref_mix.dim() != 2 or ref_mix.shape[0] != 2:
            raise ValueError(f"ref_mix must be (2, n_samples) or an AudioFeatureProfile, got {tuple(ref_mix.shape)}")
        _hip.require_same_device(tracks.device, ref_mix.data if is_profile else ref_mix)
        if int(n_iters) < 1:
            raise ValueError("n_iters must be at least 1")
        dev = tracks.device
        self.console, self.loss_function, self.callback = mix_console, loss_function, callback
        self.flags = dict(use_fx_bus=False)
        self.flags.update(console_flags)
        self.tracks = tracks.detach().unsqueeze(0)
        if is_profile:
            self.ref_mix = ref_mix
        else:
            self.ref_mix = ref_mix.detach().unsqueeze(0)
            if ref_mix.shape[1] != tracks.shape[1] and hasattr(loss_function, "profile"):
                # a reference of another length (the usual case: it is another song) is analysed here, once; the loop gets the profile
                self.ref_mix = loss_function.profile(self.ref_mix)
        self.n_iters = int(n_iters)
        self.hyper = (float(lr), float(betas[0]), float(betas[1]), float(eps))
        start = start_point(tracks.shape[0], mix_console, init_scale, generator)
        # the shapes the console takes: (1, T, 27), (1, 25), (1, 26)
        self.logits = tuple(t.to(device=dev, dtype=torch.float32).reshape((1,) + (t.shape if i == 0 else t.shape[1:])).contiguous()
                            for i, t in enumerate(start))
        self.params = tuple(torch.empty_like(t).requires_grad_(True) for t in self.logits)  # leaves the kernel rewrites
        self.state = _init(self.logits, self.params)
        self.one = torch.ones((), dtype=torch.float32, device=dev)
        self.keys, self.history, self.result = None, None, None

    def iterate(self, n):
        lib = _hip.lib()
        self.result = result = self.console(self.tracks, *self.params, **self.flags)
        losses = self.loss_function(result[1], self.ref_mix)
        keys, terms = (tuple(losses), list(losses.values())) if isinstance(losses, dict) else ((), [losses])
        if self.keys is None:
            if not 1 <= len(terms) <= _cabi.OPT_MAX_TERMS:
                raise ValueError(f"the loss must return 1..{_cabi.OPT_MAX_TERMS} terms, got {len(terms)}")
            self.keys = keys
            self.history = torch.empty(self.n_iters, 1 + len(terms), dtype=torch.float32, device=self.tracks.device)
        elif keys != self.keys:
            raise ValueError(f"the loss returned {keys} after {self.keys}: its terms must not change between iterations")
        for t in terms:
            if not isinstance(t, torch.Tensor) or t.numel() != 1 or t.dtype != torch.float32 or not t.is_cuda:
                raise TypeError("every loss term must be a one-element float32 device tensor")
        grads = torch.autograd.grad(terms, self.params, [self.one.expand(t.shape) for t in terms], allow_unused=True)
        grads = tuple(None if g is None else g.float().contiguous() for g in grads)
        if self.callback is not None:
            self.callback(n, SimpleNamespace(params=self.params, grads=grads, losses=dict(zip(keys, terms)) if keys else terms[0],
                                             logits=self.logits))
        term_ptrs = (ctypes.c_void_p * len(terms))(*[t.data_ptr() for t in terms])
        row = self.history.data_ptr() + 4 * n * self.history.shape[1]
        with _hip.launch_on(self.tracks.device) as st:
            lib.mst_logit_adam_step(_segments(self.logits, self.params, grads), len(self.logits), term_ptrs, len(terms), row,
                                    *self.hyper, self.state, st)

    def finish(self):
        history = self.history.cpu()  # the one wait of the run
        t, status, where, _ = self.state[:4].tolist()
        if status:
            raise FloatingPointError(f"optimize: a loss term or a gradient was not finite at iteration {where}; the parameters were "
                                     f"left as they stood ({t} updates applied)")
        names = ("loss",) + self.keys
        loss_history = {name: history[:, i].tolist() for i, name in enumerate(names)}
        _, mix, track_dict, fx_dict, master_dict = self.result
        lt, lf, lm = self.logits
        return mix.detach().squeeze(0), lt, track_dict, lf, fx_dict, lm, master_dict, loss_history


def optimize(tracks, ref_mix, mix_console, loss_function, init_scale=0.001, lr=1e-3, n_iters=100, *, betas=(0.9, 0.999), eps=1e-8,
             generator=None, callback=None, **console_flags):
    """The reference's ``optimize`` (scripts/online.py:15-123): fit the console's parameters to ``ref_mix`` by Adam on their logits.

    ``tracks (T, N)`` and ``ref_mix (2, M)`` are device tensors (a CPU tensor raises, as everywhere in this package).  Every iteration
    calls ``mix_console(tracks[None], p_tracks, p_fx, p_master, use_fx_bus=False, **console_flags)`` with ``p = sigmoid(logits)`` and
    ``loss_function(mix, target)`` - a dictionary of one-element terms, summed in its order like the script's ``loss += value``,
    or a single tensor - takes ``torch.autograd.grad`` of the terms with respect to the three ``p`` and hands the rest to one kernel
    launch.

    The ``target`` of every iteration: with ``M == N`` it is ``ref_mix[None]``.  With ``M != N`` (the reference mix is another song: the
    script's own ``ref_mix[:, start:start + block]`` comes out shorter whenever that song ends early) and a ``loss_function`` that has a
    ``profile`` method (``AudioFeatureLoss``), ``loss_function.profile(ref_mix[None])`` is taken once, before the first iteration,
    and every iteration gets that ``AudioFeatureProfile``; any other loss function is handed ``ref_mix[None]`` as it is and decides
    itself.  ``ref_mix`` may also BE an ``AudioFeatureProfile`` of batch size 1 - a stored one, or ``loss_function.profile(ref_mix[None])``
    of an equal-length reference (``profile`` takes ``(bs, 2, n)``), which spares the loop the target's half of the loss forward (an
    equal-length tensor keeps the paired kernels, as it always has).

    Returns the script's 8-tuple

        ``(mix, track_logits, track_param_dict, fx_bus_logits, fx_bus_param_dict, master_bus_logits, master_bus_param_dict, loss_history)``

    with ``mix (2, N)`` and the three dictionaries from the LAST iteration's forward, i.e. before the last update, as in the script; the
    logits after the last update; and ``loss_history`` a dict of Python float lists, ``"loss"`` first, then the loss dictionary's keys
    (``"loss"`` alone for a loss that returns a tensor).

    One deliberate deviation: the script returns the two bus tensors as ``(1, 1, 25)`` and ``(1, 1, 26)``; here the logits have the
    shapes this console accepts, ``(1, T, 27)``, ``(1, 25)`` and ``(1, 26)``.

    The start point is ``start_point()``: the script's three host draws, from the global generator or ``generator``.  The history
    lives on the device and is read once after the loop, followed by the optimiser's status word: if a loss term or a gradient was
    not finite at some iteration, that iteration changed nothing (torch would have spread the NaN through every parameter) and
    ``FloatingPointError`` names the first such iteration.  ``callback(n, view)`` runs after the backward and before the step of
    iteration ``n``; ``view.params``, ``view.grads``, ``view.losses`` and ``view.logits`` are the live tensors (clone what is to be kept;
    a callback that reads values synchronises, which is then the caller's choice).  A console built with ``validate="deferred"`` keeps
    the loop free of host waits; the default ``validate="sync"`` waits for its range check in every forward.
    """
    run = _Run(tracks, ref_mix, mix_console, loss_function, init_scale, lr, n_iters, betas, eps, generator, callback, console_flags)
    for n in range(run.n_iters):
        run.iterate(n)
    return run.finish()


def render_blocks(tracks, track_params, fx_bus_params, master_bus_params, mix_console, block_size=524288, **console_flags):
    """The script's "full mix generation" (scripts/online.py:325-346) on the device: ``floor(n / block_size)`` independent console
    forwards under ``no_grad`` with the sigmoid of the three logit tensors, each written into a ``(2, n)`` device tensor; the remainder
    stays zero, as in the script.  ``tracks (T, n)``; the logits as ``optimize`` returns them.  No block is copied to the host."""
    _hip.require_cuda(tracks, track_params, fx_bus_params, master_bus_params)
    if tracks.dim() != 2:
        raise ValueError(f"tracks must be (n_tracks, n_samples), got {tuple(tracks.shape)}")
    block_size = int(block_size)
    if block_size < 1:
        raise ValueError("block_size must be positive")
    n_tracks, n = tracks.shape
    flags = dict(use_fx_bus=False)
    flags.update(console_flags)
    shapes = ((1, n_tracks, mix_console.num_track_control_params), (1, mix_console.num_fx_bus_control_params),
              (1, mix_console.num_master_bus_control_params))
    with torch.no_grad():
        logits = tuple(t.detach().to(device=tracks.device, dtype=torch.float32).reshape(shape).contiguous()
                       for t, shape in zip((track_params, fx_bus_params, master_bus_params), shapes))
        params = tuple(torch.empty_like(t) for t in logits)
        _init(logits, params)
        full_mix = torch.zeros(2, n, dtype=torch.float32, device=tracks.device)
        for b in range(n // block_size):
            block = tracks[:, b * block_size:(b + 1) * block_size]
            if block.data_ptr() % 16 or block.stride(0) % 4:  # the console reads rows 16 bytes at a time
                block = block.contiguous()
            full_mix[:, b * block_size:(b + 1) * block_size] = mix_console(block.unsqueeze(0), *params, **flags)[1][0]
    return full_mix
