"""Per-song mix optimisation on the device: ``optimize()`` and the block renderer of the reference's ``scripts/online.py``, and
``optimize_batch()`` / ``pick()``: many such fits in the launches of one.

``optimize`` fits the console's parameters to a reference mix by gradient descent on their logits - no model involved (reference
scripts/online.py:15-123).  The console, the loss and their backwards are the package's kernels; everything the script does around them
per iteration (three sigmoids and their backwards, the sum of the loss dictionary, ``zero_grad``, torch's Adam over three small
tensors, six ``.item()`` host reads) is ONE launch here, ``mst_logit_adam_step`` (csrc/mst_opt.hip, include/diffmst_hip.h): it chains
dL/dp through the sigmoid, applies Adam, writes the next iteration's parameters, appends the loss terms to a history on the device and
keeps the step count there.  The host reads nothing between the first and the last iteration.

``keep_best=True`` returns the best iterate instead of the last, ``patience`` freezes a fit that has stopped improving and ``best_of()``
picks the best restart of a batch: ``mst_logit_adam_step_best`` / ``_step_best_batch`` keep the best logits in a second block on the
device inside the same one launch.

``optimize_sections`` fits ONE parameter set through several sections of a song pooled into one feature vector, and
``optimize_sections_batch`` runs a batch of such fits - restarts, several references - in the launches of one.

``pick_sections`` says where those sections should start: it meters every window of the song once on the device and picks windows in
which, between them, every track plays (``mst_loudness_windows``, ``mst_pick_sections``).

``links`` / ``stereo_id`` on all four tie the two mono rows of a stereo stem to one set of logits with a mirrored pan.

PARITY UNPINNED: the script cannot be imported (it imports ``StereoCLAPLoss``, which the reference's ``mst/loss.py`` does not define),
so its loop is restated here and checked against ``torch.optim.Adam`` behind ``torch.sigmoid`` on recorded gradients.
"""
from __future__ import annotations

import ctypes
import inspect
import struct
from collections.abc import Mapping
from types import SimpleNamespace
from typing import NamedTuple

import torch

from . import _cabi, _desc, _hip, utils
from .loss import AudioFeatureProfile


class FitReport(NamedTuple):
    """What ``keep_best=True`` appends to a result: numbers for ``optimize``, lists of ``B`` of them for ``optimize_batch``.

    ``best_iteration`` is the iteration whose loss was the best (``None`` for an item of a batch that never had a finite iteration),
    ``best_loss`` that loss (``"loss"`` of the history at that iteration; ``inf`` without a best), ``settled_at`` the iteration at
    which ``patience`` ran out (``None`` if it did not) and ``iterations_run`` the number of iterations the loop ran."""
    best_iteration: object
    best_loss: object
    settled_at: object
    iterations_run: object


def _check_best(keep_best, patience, min_delta, poll_every):
    """The four keywords of the best-iterate flow -> (patience as the kernel takes it, min_delta, poll_every or None)."""
    min_delta = float(min_delta)
    try:
        finite = 0.0 <= struct.unpack("f", struct.pack("f", min_delta))[0] < float("inf")  # the kernel compares in fp32
    except OverflowError:
        finite = False
    if not finite:
        raise ValueError(f"min_delta must be a finite fp32 number >= 0, got {min_delta}")
    if patience is not None:
        if not keep_best:
            raise ValueError("patience needs keep_best=True: an item that is frozen is returned at its best iterate")
        if int(patience) != patience or int(patience) < 0:
            raise ValueError(f"patience must be a number of iterations >= 0 (0 never freezes), got {patience}")
    elif min_delta and not keep_best:
        raise ValueError("min_delta needs keep_best=True")
    if poll_every is not None:
        if patience is None:
            raise ValueError("poll_every needs patience: without it no item ever settles")
        if int(poll_every) != poll_every or int(poll_every) < 1:
            raise ValueError(f"poll_every must be a positive number of iterations, got {poll_every}")
        poll_every = int(poll_every)
    return (0 if patience is None else int(patience)), min_delta, poll_every


def start_point(n_tracks: int, mix_console, init_scale: float = 0.001, generator=None):
    """The script's three host draws (scripts/online.py:39-45), in its order and with its shapes: ``init_scale * torch.randn`` of
    ``(n_tracks, 27)``, ``(1, 25)`` and ``(1, 26)`` from the global generator or ``generator`` - after ``torch.manual_seed(s)`` the
    start point is the script's.  Host tensors."""
    shapes = ((n_tracks, mix_console.num_track_control_params), (1, mix_console.num_fx_bus_control_params),
              (1, mix_console.num_master_bus_control_params))
    return tuple(init_scale * torch.randn(shape, generator=generator) for shape in shapes)


def links_from_stereo_id(stereo_id):
    """The reference's ``stereo_info`` flags -> the leader list ``optimize(..., links=...)`` takes.  ``stereo_id`` is a length-``T``
    sequence or 1-D tensor; a non-zero entry at row ``t`` says that row ``t + 1`` is the other channel of the same stem (the loaders
    split a stereo stem into two mono rows: reference scripts/online.py:229-240, mst/dataloader.py:321-336).  Row ``t + 1`` then
    follows row ``t``; it is skipped when the flags are walked, as mst/mixing.py:268-722 skips it, and a flag on the last row has no
    partner and is ignored (mst/mixing.py:280-283).  -> ``leader[r]``: the row whose settings row ``r`` shares, ``r`` itself if none."""
    flags = stereo_id.tolist() if isinstance(stereo_id, torch.Tensor) else list(stereo_id)
    if isinstance(stereo_id, torch.Tensor) and stereo_id.dim() != 1:
        raise ValueError(f"stereo_id must be a sequence or a 1-D tensor of flags, got shape {tuple(stereo_id.shape)}")
    leader, t = list(range(len(flags))), 0
    while t < len(flags):
        if flags[t] and t + 1 < len(flags):
            leader[t + 1] = t
            t += 2
        else:
            t += 1
    return leader


def _check_links(links, stereo_id, mirror_pan, tracks, mix_console):
    """The three keywords of a linked fit, before anything touches the device -> None without links, else the C ABI's description of
    the track segment: (rows, cols, mirror_col, leader list)."""
    if links is None and stereo_id is None:
        return None
    if links is not None and stereo_id is not None:
        raise ValueError("give links or stereo_id, not both")
    if not isinstance(tracks, torch.Tensor) or tracks.dim() < 2:
        raise ValueError("links need tracks of shape (..., n_tracks, n_samples)")
    n_tracks = tracks.shape[-2]
    if stereo_id is not None:
        links = links_from_stereo_id(stereo_id)
        what = "stereo_id"
    else:
        links = links.tolist() if isinstance(links, torch.Tensor) else list(links)
        what = "links"
    if len(links) != n_tracks:
        raise ValueError(f"{what} must have one entry per track ({n_tracks}), got {len(links)}")
    if n_tracks > _cabi.OPT_MAX_LINK_ROWS:
        raise ValueError(f"a linked fit takes at most {_cabi.OPT_MAX_LINK_ROWS} tracks, got {n_tracks}")
    for r, l in enumerate(links):
        if int(l) != l or not 0 <= l <= r or links[int(l)] != l:
            raise ValueError(f"links[{r}] = {l}: a leader is a row at or before its follower that leads itself")
    links = [int(l) for l in links]
    cols, mirror_col = mix_console.num_track_control_params, -1
    if mirror_pan:
        if cols != len(_desc.TRACK_INDEX):
            raise ValueError(f"mirror_pan needs a console with {len(_desc.TRACK_INDEX)} track parameters (its pan column is mirrored); "
                             f"{type(mix_console).__name__} has {cols}: pass mirror_pan=False")
        if any(links.count(l) > 2 for l in set(links)):
            raise ValueError("mirror_pan needs groups of at most two rows (a stereo pair): a pan has one mirror image")
        mirror_col = _desc.TRACK_INDEX.index(("stereo_panner", "pan"))
    return n_tracks, cols, mirror_col, links


def _links_struct(links):
    out = _cabi.LogitAdamLinks(segment=0, rows=links[0], cols=links[1], mirror_col=links[2])
    for r, l in enumerate(links[3]):
        out.leader[r] = l
    return out


def _segments(logits, params, grads):
    """The segment table of one call: a NULL gradient for a parameter the loss does not reach."""
    seg = (_cabi.LogitAdamSegment * len(logits))()
    for s, (theta, p, g) in zip(seg, zip(logits, params, grads)):
        s.theta, s.p, s.grad_p, s.count = theta.data_ptr(), p.data_ptr(), None if g is None else g.data_ptr(), theta.numel()
    return seg


def _init(logits, params, items=None, sections=None, links=None):
    """p <- sigmoid(logits) by the kernel every later p comes from, and a zeroed optimiser state: one block, or with ``items`` one
    block per item of the leading dimension.  With ``sections`` one block, and ``params`` has that many equal rows per logit row;
    with both, one block per item and ``items * sections`` rows, item-major.  With ``links`` (a ``LogitAdamLinks``) the follower rows
    of the track logits are first overwritten with their leaders' (DESIGN 25): one launch for every combination of the above."""
    lib = _hip.lib()
    dev = logits[0].device
    total = sum(t.numel() for t in logits)
    none = (None,) * len(logits)
    if items is None:
        nbytes = lib.mst_logit_adam_state_bytes(total)
    else:
        nbytes = lib.mst_logit_adam_batch_state_bytes(items, total // items)
    if nbytes == 0:
        raise ValueError(f"more parameters per fit than the logit-Adam kernel takes (2^20), or more than {_cabi.OPT_MAX_ITEMS} fits")
    state = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    with _hip.launch_on(dev) as st:
        if links is not None:
            lib.mst_logit_adam_init_linked(_segments(logits, params, none), len(logits), items or 1, sections or 1, links, state, st)
        elif sections is not None and items is not None:
            lib.mst_logit_adam_init_sections_batch(_segments(logits, params, none), len(logits), items, sections, state, st)
        elif sections is not None:
            lib.mst_logit_adam_init_sections(_segments(logits, params, none), len(logits), sections, state, st)
        elif items is None:
            lib.mst_logit_adam_init(_segments(logits, params, none), len(logits), state, st)
        else:
            lib.mst_logit_adam_init_batch(_segments(logits, params, none), len(logits), items, state, st)
    return state


def _check_single(tracks, ref_mix, is_profile):
    _hip.require_cuda(tracks, ref_mix.data if is_profile else ref_mix)
    if tracks.dim() != 2:
        raise ValueError(f"tracks must be (n_tracks, n_samples), got {tuple(tracks.shape)} (one song per call: no batch dimension)")
    if is_profile:
        if ref_mix.batch_size != 1:
            raise ValueError(f"a profile given as ref_mix must have batch size 1, got {ref_mix.batch_size}")
    elif ref_mix.dim() != 2 or ref_mix.shape[0] != 2:
        raise ValueError(f"ref_mix must be (2, n_samples) or an AudioFeatureProfile, got {tuple(ref_mix.shape)}")
    return None


def _is_paired(loss_function):
    """A paired loss compares the mix with the reference sample against sample (``MultiResolutionSTFTLoss``): it has no ``profile``
    method and says so with ``paired = True``.  A sectioned fit hands it the reference itself, which must then be cut like the tracks.
    (The attribute, not the missing method alone, decides: a loss with ``pooled`` and neither of the two keeps the reference forms
    and the errors it has always had.)"""
    return not hasattr(loss_function, "profile") and bool(getattr(loss_function, "paired", False))


def _check_paired_needs_no_profile(name, method, ref_mix, is_profile, loss_function, n_samples=None):
    """What only a loss with a ``profile`` method can be fitted to - a stored ``AudioFeatureProfile``, or (``n_samples`` given: the
    fits that would profile it) a reference of another length than the tracks - is refused for a paired loss as the missing method
    it is, before anything touches the device."""
    if not _is_paired(loss_function):
        return
    cls = type(loss_function).__name__
    if is_profile:
        raise TypeError(f"{name}: {cls}.{method} is paired (sample against sample) and takes a reference tensor, not an "
                        f"AudioFeatureProfile: a profile needs a loss_function with a profile method (AudioFeatureLoss), {cls} has none")
    if n_samples is not None and ref_mix.shape[-1] != n_samples:
        raise TypeError(f"{name}: a reference of {ref_mix.shape[-1]} samples against tracks of {n_samples} has to be profiled, which needs "
                        f"a loss_function with a profile method (AudioFeatureLoss): {cls} has none - {cls}.{method} is paired (sample "
                        "against sample) and takes a reference of the tracks' length")


def _check_batch(tracks, ref_mix, is_profile, loss_function, init_scale, batch):
    """Types and shapes of ``optimize_batch``, before anything touches the device -> (B, init scales)."""
    if not callable(getattr(loss_function, "per_item", None)):
        raise TypeError("optimize_batch needs a loss_function with a per_item(input, target) method (AudioFeatureLoss.per_item, "
                        f"MultiResolutionSTFTLoss.per_item): {type(loss_function).__name__} has none")
    if not isinstance(tracks, torch.Tensor) or tracks.dim() not in (2, 3):
        raise ValueError("tracks must be (B, n_tracks, n_samples), or (n_tracks, n_samples) with batch=B")
    if tracks.dim() == 3:
        if batch is not None and int(batch) != tracks.shape[0]:
            raise ValueError(f"batch={batch} with tracks of batch size {tracks.shape[0]}")
        B = tracks.shape[0]
    elif batch is None:
        raise ValueError("tracks of shape (n_tracks, n_samples) need batch=B (the song is repeated B times)")
    else:
        B = int(batch)
    if not 1 <= B <= _cabi.OPT_MAX_ITEMS:
        raise ValueError(f"the batch size must be 1..{_cabi.OPT_MAX_ITEMS}, got {B}")
    if is_profile:
        if ref_mix.batch_size not in (1, B):
            raise ValueError(f"a profile given as ref_mix must have batch size {B} or 1, got {ref_mix.batch_size}")
    elif not (ref_mix.dim() == 2 and ref_mix.shape[0] == 2) and not (ref_mix.dim() == 3 and tuple(ref_mix.shape[:2]) == (B, 2)):
        raise ValueError(f"ref_mix must be ({B}, 2, n_samples), (2, n_samples) or an AudioFeatureProfile, got {tuple(ref_mix.shape)}")
    _check_paired_needs_no_profile("optimize_batch", "per_item", ref_mix, is_profile, loss_function, tracks.shape[-1])
    if isinstance(init_scale, (int, float)):
        scales = [float(init_scale)] * B
    else:
        scales = [float(v) for v in init_scale]
        if len(scales) != B:
            raise ValueError(f"init_scale must be a number or a sequence of {B} numbers, got {len(scales)}")
    _hip.require_cuda(tracks, ref_mix.data if is_profile else ref_mix)
    return B, scales


def _check_paired_sections(ref_mix, loss_function, S, n_samples, B=None):
    """The reference of a sectioned fit under a paired loss, before anything touches the device: ``(S, 2, n)`` - one for every item of
    a batch - or, for a batch, ``(B, S, 2, n)``."""
    shape, forms = tuple(ref_mix.shape), f"({S}, 2, {n_samples})"
    if B is not None:
        forms += f" or ({B}, {S}, 2, {n_samples})"
    if shape != (S, 2, n_samples) and (B is None or shape != (B, S, 2, n_samples)):
        raise ValueError(f"{type(loss_function).__name__} is a paired loss (sample against sample: it has no profile) and needs a "
                         f"reference cut like the tracks: ref_mix {forms}, as take_sections cuts a (2, n_samples) reference with the "
                         f"tracks' starts and length - got {shape}")


def _check_sections(tracks, ref_mix, is_profile, loss_function):
    """Types and shapes of ``optimize_sections``, before anything touches the device -> S."""
    if not callable(getattr(loss_function, "pooled", None)):
        raise TypeError("optimize_sections needs a loss_function with a pooled(input, target) method (AudioFeatureLoss.pooled, "
                        f"MultiResolutionSTFTLoss.pooled): {type(loss_function).__name__} has none")
    if not isinstance(tracks, torch.Tensor) or tracks.dim() != 3:
        raise ValueError("tracks must be (S, n_tracks, n_samples): S sections of one song (take_sections cuts them)")
    S = tracks.shape[0]
    if not 1 <= S <= _cabi.OPT_MAX_SECTIONS:
        raise ValueError(f"the number of sections must be 1..{_cabi.OPT_MAX_SECTIONS}, got {S}")
    _check_paired_needs_no_profile("optimize_sections", "pooled", ref_mix, is_profile, loss_function)
    if _is_paired(loss_function):
        _check_paired_sections(ref_mix, loss_function, S, tracks.shape[-1])
    elif is_profile:
        if ref_mix.batch_size != 1:
            raise ValueError(f"a profile given as ref_mix must have batch size 1, got {ref_mix.batch_size}")
    elif not (ref_mix.dim() == 2 and ref_mix.shape[0] == 2) and not (ref_mix.dim() == 3 and ref_mix.shape[1] == 2):
        raise ValueError("ref_mix must be (2, n_samples), (R, 2, n_samples) - R sections of one reference - or an "
                         f"AudioFeatureProfile, got {tuple(ref_mix.shape)}")
    _hip.require_cuda(tracks, ref_mix.data if is_profile else ref_mix)
    return S


def _takes_items(pooled):
    """Whether ``pooled`` can be called as ``pooled(input, target, items=B)``."""
    try:
        params = inspect.signature(pooled).parameters.values()
    except (TypeError, ValueError):  # no signature to look at: the call itself will tell
        return True
    return any(p.kind is p.VAR_KEYWORD or (p.name == "items" and p.kind is not p.POSITIONAL_ONLY) for p in params)


def _check_sections_batch(tracks, ref_mix, is_profile, loss_function, init_scale, batch):
    """Types and shapes of ``optimize_sections_batch``, before anything touches the device -> (B, S, init scales)."""
    pooled = getattr(loss_function, "pooled", None)
    if not callable(pooled) or not _takes_items(pooled):
        raise TypeError("optimize_sections_batch needs a loss_function with a pooled(input, target, items=B) method "
                        f"(AudioFeatureLoss.pooled, MultiResolutionSTFTLoss.pooled): {type(loss_function).__name__} has none")
    if not isinstance(tracks, torch.Tensor) or tracks.dim() not in (3, 4):
        raise ValueError("tracks must be (B, S, n_tracks, n_samples), or (S, n_tracks, n_samples) with batch=B")
    if tracks.dim() == 4:
        if batch is not None and int(batch) != tracks.shape[0]:
            raise ValueError(f"batch={batch} with tracks of batch size {tracks.shape[0]}")
        B = tracks.shape[0]
    elif batch is None:
        raise ValueError("tracks of shape (S, n_tracks, n_samples) need batch=B (the sectioned song is repeated B times)")
    else:
        B = int(batch)
    S = tracks.shape[-3]
    if not 1 <= B <= _cabi.OPT_MAX_ITEMS:
        raise ValueError(f"the batch size must be 1..{_cabi.OPT_MAX_ITEMS}, got {B}")
    if not 1 <= S <= _cabi.OPT_MAX_SECTIONS:
        raise ValueError(f"the number of sections must be 1..{_cabi.OPT_MAX_SECTIONS}, got {S}")
    _check_paired_needs_no_profile("optimize_sections_batch", "pooled", ref_mix, is_profile, loss_function)
    if _is_paired(loss_function):
        _check_paired_sections(ref_mix, loss_function, S, tracks.shape[-1], B)
    elif is_profile:
        if ref_mix.batch_size not in (1, B):
            raise ValueError(f"a profile given as ref_mix must have batch size {B} or 1, got {ref_mix.batch_size}")
    elif not (ref_mix.dim() == 2 and ref_mix.shape[0] == 2) and not (ref_mix.dim() == 3 and tuple(ref_mix.shape[:2]) == (B, 2)) and not (
            ref_mix.dim() == 4 and ref_mix.shape[0] == B and ref_mix.shape[1] >= 1 and ref_mix.shape[2] == 2):
        raise ValueError(f"ref_mix must be (2, n_samples), ({B}, 2, n_samples), ({B}, R, 2, n_samples) - R sections of each item's "
                         f"reference - or an AudioFeatureProfile, got {tuple(ref_mix.shape)}")
    if isinstance(init_scale, (int, float)):
        scales = [float(init_scale)] * B
    else:
        scales = [float(v) for v in init_scale]
        if len(scales) != B:
            raise ValueError(f"init_scale must be a number or a sequence of {B} numbers, got {len(scales)}")
    _hip.require_cuda(tracks, ref_mix.data if is_profile else ref_mix)
    return B, S, scales


def _first_sections(value, B, S):
    """Section 0 of every item of what a console at batch ``B * S`` returned: rows ``b * S`` of every tensor, through dictionaries."""
    if isinstance(value, Mapping):  # a console built with param_dicts="lazy" fills its dictionaries here, after the loop
        return {k: _first_sections(v, B, S) for k, v in value.items()}
    return value[::S] if isinstance(value, torch.Tensor) and value.dim() >= 1 and value.shape[0] == B * S else value


class _Run:
    """One optimisation, or with ``batch`` a batch of independent ones in the same launches: set-up (the start point goes to the
    device), ``iterate(n)`` (nothing in it waits for the device) and ``finish()`` (the one read of history and status).  ``sectioned``
    gives every parameter set ``S`` sections; with ``batched`` as well, ``items`` and ``sections`` are both set."""

    def __init__(self, tracks, ref_mix, mix_console, loss_function, init_scale, lr, n_iters, betas, eps, generator, callback, console_flags,
                 batch=None, batched=False, keep_best=False, patience=None, min_delta=0.0, poll_every=None, sectioned=False, links=None,
                 stereo_id=None, mirror_pan=True):
        self.keep_best = bool(keep_best)
        self.patience, self.min_delta, self.poll_every = _check_best(self.keep_best, patience, min_delta, poll_every)
        links = _check_links(links, stereo_id, mirror_pan, tracks, mix_console)
        self.links = None if links is None else _links_struct(links)  # rows of the track logits that share their settings
        is_profile = isinstance(ref_mix, AudioFeatureProfile)
        if not is_profile and not isinstance(ref_mix, torch.Tensor):
            raise TypeError(f"ref_mix must be a (2, n_samples) tensor or an AudioFeatureProfile, got {type(ref_mix).__name__}")
        self.sections = None  # S: one parameter set fitted to S sections in the launches of one (optimize_sections)
        self.name = "optimize_sections_batch" if sectioned and batched else "optimize_batch" if batched else "optimize"
        if sectioned and batched:
            self.items, self.sections, scales = _check_sections_batch(tracks, ref_mix, is_profile, loss_function, init_scale, batch)
        elif sectioned:
            self.items, self.sections = None, _check_sections(tracks, ref_mix, is_profile, loss_function)
        elif batched:
            self.items, scales = _check_batch(tracks, ref_mix, is_profile, loss_function, init_scale, batch)
        else:
            self.items = _check_single(tracks, ref_mix, is_profile)
        B = self.items
        _hip.require_same_device(tracks.device, ref_mix.data if is_profile else ref_mix)
        if int(n_iters) < 1:
            raise ValueError("n_iters must be at least 1")
        dev = tracks.device
        self.console, self.loss_function, self.callback = mix_console, loss_function, callback
        self.flags = dict(use_fx_bus=False)
        self.flags.update(console_flags)
        n_tracks, n_samples = tracks.shape[-2:]
        if self.sections is not None and B is not None:  # (B * S, T, n), item-major: row b * S + s is section s of item b
            rows = tracks.detach() if tracks.dim() == 4 else tracks.detach().unsqueeze(0).repeat(B, 1, 1, 1)
            self.tracks = rows.reshape(B * self.sections, n_tracks, n_samples).contiguous()
        elif self.sections is not None:
            self.tracks = tracks.detach()
        elif B is None:
            self.tracks = tracks.detach().unsqueeze(0)
        else:
            self.tracks = tracks.detach() if tracks.dim() == 3 else tracks.detach().unsqueeze(0).repeat(B, 1, 1)
        if is_profile:
            self.ref_mix = ref_mix
        elif self.sections is not None and B is not None:
            # analysed here, once: one reference for every item, one per item, or one per item given as R sections and pooled
            ref = ref_mix.detach()
            if _is_paired(loss_function):
                # a paired loss has no profile: it gets the reference itself, flattened item-major like the mix it meets, (B S, 2, n)
                rows = ref if ref.dim() == 4 else ref.unsqueeze(0).expand(B, -1, -1, -1)
                self.ref_mix = rows.reshape(B * self.sections, 2, n_samples).contiguous()
            elif ref.dim() == 4:
                self.ref_mix = loss_function.profile(ref.reshape((-1,) + tuple(ref.shape[2:])), pool=True, items=B)
            else:
                self.ref_mix = loss_function.profile(ref.unsqueeze(0) if ref.dim() == 2 else ref)
        elif self.sections is not None:
            # the pooled loss has no paired route: the reference is analysed here, once - its sections pooled if it comes as sections
            ref = ref_mix.detach()
            if _is_paired(loss_function):  # the reference itself, (S, 2, n): section s of it meets section s of the mix
                self.ref_mix = ref.contiguous()
            else:
                self.ref_mix = loss_function.profile(ref, pool=True) if ref.dim() == 3 else loss_function.profile(ref.unsqueeze(0))
        else:
            self.ref_mix = ref_mix.detach()
            if self.ref_mix.dim() == 2:
                self.ref_mix = self.ref_mix.unsqueeze(0)
            if (B is not None or ref_mix.shape[-1] != n_samples) and hasattr(loss_function, "profile"):
                # a reference of another length (the usual case: it is another song) is analysed here, once; the loop gets the profile.
                # A batch always takes the profile: its loss has no paired route
                self.ref_mix = loss_function.profile(self.ref_mix)
            elif B is not None and self.ref_mix.shape[0] != B:
                self.ref_mix = self.ref_mix.expand(B, -1, -1)
        self.n_iters = int(n_iters)
        self.hyper = (float(lr), float(betas[0]), float(betas[1]), float(eps))
        if B is None:
            start = start_point(n_tracks, mix_console, init_scale, generator)
            # the shapes the console takes: (1, T, 27), (1, 25), (1, 26)
            self.logits = tuple(t.to(device=dev, dtype=torch.float32).reshape((1,) + (t.shape if i == 0 else t.shape[1:])).contiguous()
                                for i, t in enumerate(start))
        else:
            # item b starts at the b-th successive draw, so B = 1 starts where optimize() does: (B, T, 27), (B, 25), (B, 26)
            draws = [start_point(n_tracks, mix_console, scale, generator) for scale in scales]
            self.logits = tuple(torch.stack([d[i] if i == 0 else d[i][0] for d in draws]).to(device=dev, dtype=torch.float32).contiguous()
                                for i in range(3))
        if self.sections is None:
            self.params = tuple(torch.empty_like(t).requires_grad_(True) for t in self.logits)  # leaves the kernel rewrites
        else:  # (S, T, 27), (S, 25), (S, 26) leaves whose rows the kernel keeps equal: the console runs at batch S - or, for a batch
            # of sectioned fits, (B S, ...) leaves whose rows are equal within an item: the console runs at batch B S
            self.params = tuple(torch.empty(((B or 1) * self.sections,) + t.shape[1:], dtype=t.dtype, device=dev).requires_grad_(True)
                                for t in self.logits)
        self.state = _init(self.logits, self.params, B, self.sections, self.links)
        self.best = None
        if self.keep_best:  # all zero: no best yet
            per_item = sum(t.numel() for t in self.logits) // (B or 1)
            self.best = torch.zeros(_hip.lib().mst_logit_adam_best_bytes(B or 1, per_item) // 4, dtype=torch.int32, device=dev)
        self.one = torch.ones((), dtype=torch.float32, device=dev)
        self.keys, self.history, self.result, self.ran = None, None, None, 0

    def iterate(self, n):
        lib = _hip.lib()
        B = self.items
        self.result = result = self.console(self.tracks, *self.params, **self.flags)
        if self.sections is not None and B is not None:
            losses = self.loss_function.pooled(result[1], self.ref_mix, items=B)
        elif self.sections is not None:
            losses = self.loss_function.pooled(result[1], self.ref_mix)
        else:
            losses = (self.loss_function if B is None else self.loss_function.per_item)(result[1], self.ref_mix)
        keys, terms = (tuple(losses), list(losses.values())) if isinstance(losses, dict) else ((), [losses])
        if self.keys is None:
            if not 1 <= len(terms) <= _cabi.OPT_MAX_TERMS:
                raise ValueError(f"the loss must return 1..{_cabi.OPT_MAX_TERMS} terms, got {len(terms)}")
            self.keys = keys
            shape = (self.n_iters, 1 + len(terms)) if B is None else (self.n_iters, B, 1 + len(terms))
            self.history = torch.empty(shape, dtype=torch.float32, device=self.tracks.device)
        elif keys != self.keys:
            raise ValueError(f"the loss returned {keys} after {self.keys}: its terms must not change between iterations")
        for t in terms:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or (
                    t.numel() != 1 if B is None else tuple(t.shape) != (B,)):
                raise TypeError("every loss term must be a one-element float32 device tensor" if B is None else
                                f"every per-item loss term must be a ({B},) float32 device tensor")
        grads = torch.autograd.grad(terms, self.params, [self.one.expand(t.shape) for t in terms], allow_unused=True)
        grads = tuple(None if g is None else g.float().contiguous() for g in grads)
        if self.callback is not None:
            self.callback(n, SimpleNamespace(params=self.params, grads=grads, losses=dict(zip(keys, terms)) if keys else terms[0],
                                             logits=self.logits))
        row = self.history.data_ptr() + 4 * n * self.history[0].numel()
        segments = _segments(self.logits, self.params, grads)
        if self.links is not None:  # one call for single, batch, sections and best: the items' terms as a dense (items, n_terms)
            adjacent = B is None and all(t.data_ptr() == terms[0].data_ptr() + 4 * k for k, t in enumerate(terms))
            # (the one-element terms of a single fit usually are views of one buffer, side by side: no copy then)
            dense = terms[0] if adjacent else torch.stack([t.detach().reshape(B or 1) for t in terms], dim=1)
            with _hip.launch_on(self.tracks.device) as st:
                lib.mst_logit_adam_step_linked(segments, len(self.logits), B or 1, self.sections or 1, self.links, dense, len(terms), row,
                                               *self.hyper, self.min_delta, self.patience, self.state, self.best, st)
        elif B is None:
            term_ptrs = (ctypes.c_void_p * len(terms))(*[t.data_ptr() for t in terms])
            with _hip.launch_on(self.tracks.device) as st:
                if self.sections is not None:  # the S gradient rows are summed inside the step
                    lib.mst_logit_adam_step_sections(segments, len(self.logits), self.sections, term_ptrs, len(terms), row, *self.hyper,
                                                     self.min_delta, self.patience, self.state, self.best, st)
                elif self.keep_best:
                    lib.mst_logit_adam_step_best(segments, len(self.logits), term_ptrs, len(terms), row, *self.hyper, self.min_delta,
                                                 self.patience, self.state, self.best, st)
                else:
                    lib.mst_logit_adam_step(segments, len(self.logits), term_ptrs, len(terms), row, *self.hyper, self.state, st)
        else:
            dense = torch.stack([t.detach() for t in terms], dim=1)  # (B, n_terms), after the callback: it sees what the callback left
            with _hip.launch_on(self.tracks.device) as st:
                if self.sections is not None:  # every item's S gradient rows are summed inside the step
                    lib.mst_logit_adam_step_sections_batch(segments, len(self.logits), B, self.sections, dense, len(terms), row,
                                                           *self.hyper, self.min_delta, self.patience, self.state, self.best, st)
                elif self.keep_best:
                    lib.mst_logit_adam_step_best_batch(segments, len(self.logits), B, dense, len(terms), row, *self.hyper,
                                                       self.min_delta, self.patience, self.state, self.best, st)
                else:
                    lib.mst_logit_adam_step_batch(segments, len(self.logits), B, dense, len(terms), row, *self.hyper, self.state, st)
        self.ran = n + 1

    def loop(self):
        """Every iteration, or with ``poll_every`` until every item is settled or stopped: the read every ``poll_every`` iterations
        is the one wait the caller asked for."""
        for n in range(self.n_iters):
            self.iterate(n)
            if self.poll_every and (n + 1) % self.poll_every == 0 and self.all_done():
                break
        return self.finish()

    def all_done(self):
        """Every item is settled (best word [3]) or stopped (state word [1]): a read of the device."""
        B = self.items or 1
        settled = self.best.view(B, -1)[:, 3]
        stopped = self.state.view(B, -1)[:, 1]
        return bool(((settled != 0) | (stopped != 0)).all())

    def _per_item(self, mix, *dicts):
        """What a console at batch ``B S`` returned, as a batch of sectioned fits returns it: ``mix (B, S, 2, n)`` and the
        dictionaries at batch ``B`` (section 0 of every item: all rows of an item are equal)."""
        B, S = self.items, self.sections
        return (mix.reshape((B, S) + tuple(mix.shape[1:])),) + tuple(_first_sections(d, B, S) for d in dicts)

    def _finish_best(self):
        """The best iterate in place of the last one: its logits out of the best block, its parameters by the init launch (the sigmoid
        bits the loop used), one console forward under ``no_grad`` -> (mix, logits, dictionaries, report columns, state words)."""
        B = self.items or 1
        hdr = _cabi.OPT_BEST_HEADER_WORDS
        counts = [t.numel() // B for t in self.logits]
        block = self.best.view(B, -1)
        words = block[:, :4].tolist()
        state_words = self.state.view(B, -1)[:, :4].tolist()
        has_best = [w[0] != 0 for w in words]
        if not any(has_best):
            where = [w[2] for w in state_words]
            raise FloatingPointError(f"{self.name}: no iteration had a finite loss and gradient "
                                     f"(first at iteration{'s' if self.items else ''} {where if self.items else where[0]}); the "
                                     "parameters were left as they stood")
        stored = block[:, hdr:hdr + sum(counts)].view(torch.float32).split(counts, dim=1)
        keep = torch.tensor(has_best, device=block.device)
        # an item without a best iterate never moved: its live logits are its start point
        logits = tuple(torch.where(keep.view((B,) + (1,) * (live.dim() - 1)), got.reshape(live.shape), live).contiguous()
                       for got, live in zip(stored, self.logits))
        with torch.no_grad():
            rows = (lambda t: t.shape) if self.sections is None else (lambda t: (B * self.sections,) + t.shape[1:])
            params = tuple(torch.empty(rows(t), dtype=t.dtype, device=t.device) for t in logits)
            _init(logits, params, self.items, self.sections, self.links)  # consistent already: the followers keep their bits
            _, mix, track_dict, fx_dict, master_dict = self.console(self.tracks, *params, **self.flags)
            if self.items is not None and self.sections is not None:
                mix, track_dict, fx_dict, master_dict = self._per_item(mix, track_dict, fx_dict, master_dict)
        best_loss = [struct.unpack("f", struct.pack("i", w[1]))[0] if ok else float("inf") for w, ok in zip(words, has_best)]
        report = FitReport([w[0] - 1 if ok else None for w, ok in zip(words, has_best)], best_loss,
                           [w[3] - 1 if w[3] else None for w in words], [self.ran] * B)
        return mix, logits, (track_dict, fx_dict, master_dict), report, state_words

    def finish(self):
        history = self.history[:self.ran].cpu()  # the one wait of the run
        names = ("loss",) + self.keys
        if self.keep_best:
            mix, (lt, lf, lm), (track_dict, fx_dict, master_dict), report, words = self._finish_best()
            if self.items is not None:
                stopped_at = [where if status else None for _, status, where, _ in words]
                loss_history = {name: history[:, :, i].clone() for i, name in enumerate(names)}
                return mix.detach(), lt, track_dict, lf, fx_dict, lm, master_dict, loss_history, stopped_at, report
            loss_history = {name: history[:, i].tolist() for i, name in enumerate(names)}
            if self.sections is not None:
                mix = mix.unsqueeze(0)  # squeezed again below: (S, 2, n)
            return (mix.detach().squeeze(0), lt, track_dict, lf, fx_dict, lm, master_dict, loss_history,
                    FitReport(*(column[0] for column in report)))
        _, mix, track_dict, fx_dict, master_dict = self.result
        lt, lf, lm = self.logits
        if self.items is not None:
            words = self.state.view(self.items, -1)[:, :4].tolist()
            stopped_at = [where if status else None for _, status, where, _ in words]
            if all(w is not None for w in stopped_at):
                raise FloatingPointError(f"{self.name}: every item met a loss term or a gradient that was not finite (first at "
                                         f"iterations {stopped_at}); those iterations left the parameters as they stood")
            loss_history = {name: history[:, :, i].clone() for i, name in enumerate(names)}
            if self.sections is not None:
                mix, track_dict, fx_dict, master_dict = self._per_item(mix, track_dict, fx_dict, master_dict)
            return mix.detach(), lt, track_dict, lf, fx_dict, lm, master_dict, loss_history, stopped_at
        t, status, where, _ = self.state[:4].tolist()
        if self.sections is not None:
            mix = mix.unsqueeze(0)  # squeezed again below: (S, 2, n)
        if status:
            raise FloatingPointError(f"optimize: a loss term or a gradient was not finite at iteration {where}; the parameters were "
                                     f"left as they stood ({t} updates applied)")
        loss_history = {name: history[:, i].tolist() for i, name in enumerate(names)}
        return mix.detach().squeeze(0), lt, track_dict, lf, fx_dict, lm, master_dict, loss_history


def optimize(tracks, ref_mix, mix_console, loss_function, init_scale=0.001, lr=1e-3, n_iters=100, *, betas=(0.9, 0.999), eps=1e-8,
             generator=None, callback=None, keep_best=False, patience=None, min_delta=0.0, poll_every=None, links=None,
             stereo_id=None, mirror_pan=True, **console_flags):
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

    ``keep_best=True`` returns the BEST iterate instead of the last: Adam with a fixed ``lr`` does not descend monotonically
    on this loss.  Every iteration is still one launch (``mst_logit_adam_step_best``) and nothing in the loop reads the device: the
    kernel compares the loss sum with the best so far - an improvement is ``loss < best - min_delta`` in fp32, so a tie keeps the earlier
    iterate - and on an improvement keeps the logits the loss was evaluated at.  After the loop the best logits become parameters by
    the init launch and go through one more console forward under ``no_grad``; the tuple then holds the best iterate's ``mix``, logits
    and dictionaries (``render_blocks(song, *result[1:6:2], console)`` renders the best fit), ``loss_history`` stays the whole run's,
    and a ninth element is a ``FitReport(best_iteration, best_loss, settled_at, iterations_run)``.  An iteration that was not finite
    changes nothing, as ever, and no longer raises as long as some iteration has a best to report.  ``patience=k`` (needs
    ``keep_best``) freezes the fit once ``k`` iterations in a row have not improved: later iterations write their history row and
    nothing else.  ``poll_every=j`` (needs ``patience``) makes the host read the settled word every ``j`` iterations - a wait the caller
    asks for - and leave the loop when the fit has settled; the history is as long as the iterations that ran.

    ``links`` / ``stereo_id`` tie rows of the track logits: the loaders split a stereo stem into two mono rows, and an
    unlinked fit is free to EQ, compress and fade the two halves of an overhead pair differently and to pan both to one side.
    ``links`` is a leader list of length ``T`` (``links[r]`` is the row whose settings row ``r`` shares, ``r`` itself if none;
    a leader leads itself and stands before its followers), ``stereo_id`` the reference's flags (``links_from_stereo_id``); giving both
    is a ``ValueError``.  The rows of a group share ONE set of logits: the init launch copies the leader's start point over its
    followers (all ``T`` rows are still drawn, so the generator's stream is the script's), and every step forms the gradient of a shared
    logit as the sum of its members' chained gradients, in member order in fp32, inside the same one launch
    (``mst_logit_adam_step_linked``) and writes the new logit and parameter to every member.  ``mirror_pan=True`` (groups of at most
    two rows, a console with the 27 track parameters) gives the follower MINUS the leader's pan logit, so its pan is ``1 - pan``
    (reference mst/mixing.py:268-722).  The returned logits are full ``(1, T, 27)`` tensors and already consistent.  With neither
    keyword the calls made are exactly those without this feature.  The same three keywords work in ``optimize_batch``,
    ``optimize_sections`` and ``optimize_sections_batch``; one map serves every item of a batch.
    """
    run = _Run(tracks, ref_mix, mix_console, loss_function, init_scale, lr, n_iters, betas, eps, generator, callback, console_flags,
               keep_best=keep_best, patience=patience, min_delta=min_delta, poll_every=poll_every,
               links=links, stereo_id=stereo_id, mirror_pan=mirror_pan)
    return run.loop()


def optimize_batch(tracks, ref_mix, mix_console, loss_function, init_scale=0.001, lr=1e-3, n_iters=100, *, batch=None, betas=(0.9, 0.999),
                   eps=1e-8, generator=None, callback=None, keep_best=False, patience=None, min_delta=0.0, poll_every=None,
                   links=None, stereo_id=None, mirror_pan=True, **console_flags):
    """``B`` independent ``optimize`` runs in the launches of one: random restarts, one song against several references, several songs
    against one reference.  One console forward at batch ``B``, ``loss_function.per_item``, one ``torch.autograd.grad`` with a ones
    cotangent per ``(B,)`` term and one ``mst_logit_adam_step_batch`` per iteration; nothing in the loop waits for the host.

    ``tracks`` is ``(B, T, N)``, or ``(T, N)`` with ``batch=B`` (the song is repeated).  ``ref_mix`` is ``(B, 2, M)``, ``(2, M)`` (one
    reference for every item) or an ``AudioFeatureProfile`` of batch size ``B`` or 1; a tensor is profiled once, before the loop.
    ``loss_function`` must offer ``per_item(input, target)`` -> ``(B,)`` terms (``AudioFeatureLoss.per_item``,
    ``MultiResolutionSTFTLoss.per_item``): with a batch-mean loss every item's gradient would carry ``1 / B``, which Adam's ``eps`` makes
    visible.  A loss without a ``profile`` method (the paired ``MultiResolutionSTFTLoss``: recreating an existing mix of the same
    stems, where restarts matter because the spectrogram loss is far from convex in the EQ and compressor settings) is handed the
    reference itself, ``(B, 2, N)`` - one ``(2, N)`` reference is repeated - and returns one ``(B,)`` tensor: the history then has the
    ``"loss"`` column alone; a profile, or a reference of another length than the tracks, needs the ``profile`` method such a loss
    lacks and is a ``TypeError``.  ``init_scale`` is a number or ``B`` numbers.  Item
    ``b`` starts at the ``b``-th successive ``start_point()`` draw from the generator, so ``B = 1`` starts where ``optimize`` starts.

    Returns ``optimize``'s 8-tuple with a leading batch dimension everywhere, plus ``stopped_at``: ``mix (B, 2, N)``, logits
    ``(B, T, 27)``, ``(B, 25)``, ``(B, 26)``, the console's dictionaries at batch ``B``, ``loss_history[name]`` an ``(n_iters, B)`` host
    tensor, and ``stopped_at`` a list of ``B`` entries, ``None`` or the first iteration at which that item's loss or gradient was not
    finite (such an iteration leaves the item's parameters as they stood and touches no other item).  ``FloatingPointError`` is raised
    only when every item stopped.  ``pick(result, b)`` is item ``b`` in the form ``optimize`` returns.  ``callback(n, view)`` sees the
    batched live tensors.

    ``keep_best``, ``patience``, ``min_delta`` and ``poll_every`` are ``optimize``'s, per item (``mst_logit_adam_step_best_batch``):
    every item is returned at its own best iterate, an item whose patience has run out is frozen while the others go on, and with
    ``poll_every`` the loop ends once every item is settled or stopped.  The ``FitReport`` of lists follows ``stopped_at`` as a tenth
    element; ``FloatingPointError`` is raised only when no item has a best iterate.  ``best_of(result)`` is the item with the lowest
    best loss - the random-restart recipe ranks restarts by that, not by the noise of the last step."""
    run = _Run(tracks, ref_mix, mix_console, loss_function, init_scale, lr, n_iters, betas, eps, generator, callback, console_flags,
               batch=batch, batched=True, keep_best=keep_best, patience=patience, min_delta=min_delta, poll_every=poll_every,
               links=links, stereo_id=stereo_id, mirror_pan=mirror_pan)
    return run.loop()


def take_sections(tracks, starts, length):
    """``tracks (T, N)`` -> the contiguous ``(S, T, length)`` tensor of the sections ``tracks[:, start:start + length]``, one per entry
    of ``starts``, on the device of ``tracks``: what ``optimize_sections`` takes.  A ``(2, N)`` reference mix is cut the same way, into
    the ``(S, 2, length)`` reference a paired loss (``MultiResolutionSTFTLoss``) needs beside tracks cut with the same ``starts``."""
    if not isinstance(tracks, torch.Tensor) or tracks.dim() != 2:
        raise ValueError("tracks must be (n_tracks, n_samples)")
    starts, length = [int(v) for v in starts], int(length)
    if not starts or length < 1:
        raise ValueError("take_sections needs at least one start and a positive length")
    for start in starts:
        if start < 0 or start + length > tracks.shape[1]:
            raise ValueError(f"the section [{start}, {start + length}) does not lie inside the {tracks.shape[1]} samples of the tracks")
    return torch.stack([tracks[:, start:start + length] for start in starts]).contiguous()


class SectionPick(NamedTuple):
    """What ``pick_sections`` returns.  ``starts`` is a list of Python ints in pick order and ``length`` the section length, both as
    ``take_sections`` takes them; the rest are device tensors over the ``S = len(starts)`` picked windows: ``active (S, T)`` bool - the
    tracks that play in each, ``covered (T)`` bool - the tracks that play in any, ``track_lufs (T, S)`` and ``mix_lufs (S)`` - the
    windowed loudness of the tracks and of their mono sum there."""
    starts: list
    length: int
    active: torch.Tensor
    covered: torch.Tensor
    track_lufs: torch.Tensor
    mix_lufs: torch.Tensor


def pick_sections(tracks, length, count, *, sample_rate=44100, hop=None, track_floor_lufs=-48.0, mix_floor_lufs=-48.0, min_gap=None):
    """Where the sections of a sectioned fit should start: up to ``count`` windows of ``length`` samples of ``tracks (T, N)`` in which,
    between them, every track plays.  A track that is silent in every section of a fit gets a zero gradient for all of its
    logits and keeps its start point, which ``render_blocks`` then applies to the whole song.

    The ``T`` tracks and their mono sum ``tracks.sum(0)`` are metered once each (``mst.utils.windowed_loudness``: windows every ``hop``
    samples, default ``sample_rate / 10``).  A track is active in a window when its loudness there reaches ``track_floor_lufs`` (a number
    or a ``(T,)`` tensor), a window is eligible when the sum reaches ``mix_floor_lufs`` and some track is active in it, and
    ``mst_pick_sections`` takes, ``count`` times, the eligible window at least ``min_gap`` samples (default ``length``: no two sections
    overlap) from every window taken so far that has the most active tracks not yet covered - then the most active tracks, then the
    loudest sum, then the earliest.  The -48 LUFS defaults are the thresholds the reference's data loader drops a crop at
    (mst/dataloader.py:39-69, :286-309); they apply to the tracks as they are given, BEFORE any loudness normalisation.  Windows that
    end after the last sample are not offered.  The call reads the device once, for the picked windows.

    Returns a ``SectionPick``; fewer than ``count`` sections come back as they are, none at all is a ``ValueError``.  Check
    ``pick.covered`` for tracks that play nowhere above their floor.

        pick = pick_sections(tracks, 131072, 4)
        sections = take_sections(tracks, pick.starts, pick.length)                      # (S, T, 131072)
        result = optimize_sections(sections, ref_mix, console, AudioFeatureLoss(weights, 44100))
        mix = render_blocks(tracks, result[1], result[3], result[5], console)
    """
    if not isinstance(tracks, torch.Tensor):
        raise TypeError(f"tracks must be a (n_tracks, n_samples) tensor, got {type(tracks).__name__}")
    if tracks.dim() != 2 or not tracks.is_floating_point():
        raise ValueError(f"tracks must be a floating-point (n_tracks, n_samples) tensor, got {tracks.dtype} {tuple(tracks.shape)}")
    for name, value in (("length", length), ("count", count)):
        if isinstance(value, bool) or not isinstance(value, int):
            raise TypeError(f"{name} must be an int, got {type(value).__name__}")
    T, N = tracks.shape
    if not 1 <= T <= _cabi.PICK_MAX_TRACKS:
        raise ValueError(f"the number of tracks must be 1..{_cabi.PICK_MAX_TRACKS}, got {T}")
    if not 1 <= count <= _cabi.OPT_MAX_SECTIONS:
        raise ValueError(f"count must be 1..{_cabi.OPT_MAX_SECTIONS} (what optimize_sections takes), got {count}")
    _, H, starts = utils.loudness_window_grid(N, length, hop, sample_rate)
    hop_samples = H * utils._block_step(sample_rate)
    min_gap = length if min_gap is None else min_gap
    if isinstance(min_gap, bool) or not isinstance(min_gap, int) or min_gap < 0:
        raise ValueError(f"min_gap must be a non-negative number of samples, got {min_gap!r}")
    gap = max(1, -(-min_gap // hop_samples))  # windows: the smallest distance of starts that is min_gap samples or more
    if isinstance(track_floor_lufs, torch.Tensor):
        if tuple(track_floor_lufs.shape) != (T,):
            raise ValueError(f"track_floor_lufs must be a number or a ({T},) tensor, got {tuple(track_floor_lufs.shape)}")
    else:
        track_floor_lufs = float(track_floor_lufs)
    mix_floor_lufs = float(mix_floor_lufs)
    offered = sum(1 for s in starts if s + length <= N)  # NW, or a few less when length is not a whole number of hops
    if not offered:
        raise ValueError(f"a section of {length} samples does not fit into the {N} samples of the tracks")
    _hip.require_cuda(tracks)
    dev = tracks.device
    with torch.no_grad():
        track_lufs, _ = utils.windowed_loudness(tracks.detach().unsqueeze(1), length, hop, sample_rate)
        mix_lufs, _ = utils.windowed_loudness(tracks.detach().sum(0).view(1, 1, N), length, hop, sample_rate)
        track_lufs, mix_lufs = track_lufs[:, :offered].contiguous(), mix_lufs.view(-1)[:offered].contiguous()
        if isinstance(track_floor_lufs, torch.Tensor):
            floor = track_floor_lufs.detach().to(device=dev, dtype=torch.float32).contiguous()
        else:
            floor = torch.full((T,), track_floor_lufs, dtype=torch.float32, device=dev)
        windows = torch.empty(count, dtype=torch.int32, device=dev)
        active = torch.empty(count, T, dtype=torch.uint8, device=dev)
        covered = torch.empty(T, dtype=torch.uint8, device=dev)
        with _hip.launch_on(dev) as st:
            _hip.lib().mst_pick_sections(track_lufs, mix_lufs, floor, mix_floor_lufs, T, offered, count, gap, windows, active, covered, st)
        picked = [w for w in windows.tolist() if w >= 0]  # the one host read; the -1 entries trail
        if not picked:
            raise ValueError(f"no window of {length} samples is eligible: the sum of the tracks stays below {mix_floor_lufs} LUFS or no "
                             "track reaches its floor")
        index = windows[:len(picked)].long()
        return SectionPick([starts[w] for w in picked], length, active[:len(picked)].bool(), covered.bool(),
                           track_lufs.index_select(1, index), mix_lufs.index_select(0, index))


def optimize_sections(tracks, ref_mix, mix_console, loss_function, init_scale=0.001, lr=1e-3, n_iters=100, *, betas=(0.9, 0.999),
                      eps=1e-8, generator=None, callback=None, keep_best=False, patience=None, min_delta=0.0, poll_every=None,
                      links=None, stereo_id=None, mirror_pan=True, **console_flags):
    """``optimize`` for ONE set of console parameters seen through ``S`` sections of the song at once: ``tracks`` is
    ``(S, T, n)`` (``take_sections``), the console runs at batch ``S`` with parameter leaves ``(S, T, 27)``, ``(S, 25)``, ``(S, 26)``
    whose rows are equal, ``loss_function.pooled(mix, target)`` turns the ``S`` rendered sections into ONE feature vector and one set
    of terms, autograd hands back ``(S, ...)`` gradients and ``mst_logit_adam_step_sections`` sums them in section order inside the one
    step launch - no ``expand``, no copy, no sum on the host.  The parameters that come out are applied to the whole song
    (``render_blocks``), so what they are fitted to should not be one verse: a crest factor, a stereo width or a Bark spectrum over
    several sections is compared with a target profile that was pooled over a whole reference.

    ``ref_mix`` is ``(2, M)``, ``(R, 2, M)`` - ``R`` sections of one reference, pooled - or an ``AudioFeatureProfile`` of batch size 1;
    a tensor is analysed once, before the loop.  ``loss_function`` must offer ``pooled`` (``AudioFeatureLoss``,
    ``MultiResolutionSTFTLoss``): anything else raises ``TypeError``.  A loss without a ``profile`` method (``MultiResolutionSTFTLoss``)
    is paired: its ``ref_mix`` is ``(S, 2, n)``, cut like the tracks (``take_sections`` with the same starts and length), and goes to
    ``pooled`` as it is - the ``S`` sections are one item of ``2 S`` rows; any other section count or length is a ``ValueError``
    before anything touches the device.  The keywords are ``optimize``'s, ``keep_best``, ``patience``, ``min_delta``, ``poll_every``
    and ``callback`` included (``view.params`` and ``view.grads`` have ``S`` rows).  The start point is ``optimize``'s.

    Returns ``optimize``'s tuple with ``mix (S, 2, n)``, the dictionaries at batch ``S`` and the logits in ``optimize``'s shapes
    ``(1, T, 27)``, ``(1, 25)``, ``(1, 26)``, ready for ``render_blocks``.  ``S = 1`` against a profile is ``optimize`` bit for bit."""
    run = _Run(tracks, ref_mix, mix_console, loss_function, init_scale, lr, n_iters, betas, eps, generator, callback, console_flags,
               keep_best=keep_best, patience=patience, min_delta=min_delta, poll_every=poll_every, sectioned=True,
               links=links, stereo_id=stereo_id, mirror_pan=mirror_pan)
    return run.loop()


def optimize_sections_batch(tracks, ref_mix, mix_console, loss_function, init_scale=0.001, lr=1e-3, n_iters=100, *, batch=None,
                            betas=(0.9, 0.999), eps=1e-8, generator=None, callback=None, keep_best=False, patience=None,
                            min_delta=0.0, poll_every=None, links=None, stereo_id=None, mirror_pan=True, **console_flags):
    """``B`` independent ``optimize_sections`` fits in the launches of one: restarts of a sectioned fit (``best_of`` keeps
    the best), one sectioned song against several references.  Per iteration one console forward at batch ``B S`` with parameter leaves
    ``(B S, T, 27)``, ``(B S, 25)``, ``(B S, 26)`` whose rows are equal within an item, ``loss_function.pooled(mix, target, items=B)``,
    one ``torch.autograd.grad`` with a ones cotangent per ``(B,)`` term and ONE ``mst_logit_adam_step_sections_batch``, which sums every
    item's ``S`` gradient rows in section order; nothing in the loop waits for the host.

    ``tracks`` is ``(B, S, T, n)``, or ``(S, T, n)`` with ``batch=B`` (the sectioned song is repeated: restarts).  Rows are item-major:
    the console sees row ``b S + s`` for section ``s`` of item ``b``.  ``ref_mix`` is ``(2, M)`` (one reference for every item),
    ``(B, 2, M)``, ``(B, R, 2, M)`` - every item's reference as ``R`` sections, pooled - or an ``AudioFeatureProfile`` of batch size ``B``
    or 1; a tensor is analysed once, before the loop.  ``loss_function`` must offer ``pooled`` with ``items`` (``AudioFeatureLoss``,
    ``MultiResolutionSTFTLoss``): anything else raises ``TypeError``.  For a paired loss (no ``profile`` method:
    ``MultiResolutionSTFTLoss``) ``ref_mix`` is ``(S, 2, n)`` - one reference, cut like the tracks, for every item - or ``(B, S, 2, n)``,
    flattened item-major like the mix; any other section count or length is a ``ValueError`` before anything touches the device.  ``init_scale`` is a number or ``B`` numbers; item ``b`` starts at the ``b``-th successive
    ``start_point()`` draw, as in ``optimize_batch``, so ``B = 1`` is ``optimize_sections`` and ``S = 1`` is ``optimize_batch`` against a
    profile, both bit for bit.

    Returns ``optimize_batch``'s 9-tuple (10 with ``keep_best``: the ``FitReport`` of lists): ``mix (B, S, 2, n)``, logits
    ``(B, T, 27)``, ``(B, 25)``, ``(B, 26)``, the dictionaries at batch ``B`` (section 0 of every item), ``loss_history[name]`` an
    ``(n_iters, B)`` host tensor and ``stopped_at``.  ``keep_best``, ``patience``, ``min_delta`` and ``poll_every`` work per item, a
    non-finite item stops alone, and ``FloatingPointError`` is raised only when every item stopped (with ``keep_best``: when no item has
    a best iterate).  ``pick(result, b)`` is item ``b`` as ``optimize_sections`` returns it - ``mix (S, 2, n)``, logits ready for
    ``render_blocks`` - and ``best_of(result)`` the item with the lowest best loss."""
    run = _Run(tracks, ref_mix, mix_console, loss_function, init_scale, lr, n_iters, betas, eps, generator, callback, console_flags,
               batch=batch, batched=True, keep_best=keep_best, patience=patience, min_delta=min_delta, poll_every=poll_every,
               sectioned=True,
               links=links, stereo_id=stereo_id, mirror_pan=mirror_pan)
    return run.loop()


def pick(result, b):
    """Item ``b`` of an ``optimize_batch`` result as the 8-tuple ``optimize`` returns: ``mix (2, N)``, logits ``(1, T, 27)``,
    ``(1, 25)``, ``(1, 26)`` (what ``render_blocks`` takes), the dictionaries at batch 1, the history as Python float lists.  A
    result of ``keep_best=True`` (one element longer: its ``FitReport``) is taken as well; item ``b``'s report is
    ``[column[b] for column in result[9]]``."""
    if len(result) not in (9, 10):
        raise ValueError(f"pick takes what optimize_batch returns (9 elements, 10 with keep_best), got {len(result)}")
    mix, lt, track_dict, lf, fx_dict, lm, master_dict, loss_history = result[:8]
    B = mix.shape[0]
    b = range(B)[b]  # IndexError for an item that is not there; negative indices count from the end

    def item(v):
        if isinstance(v, dict):
            return {k: item(x) for k, x in v.items()}
        return v[b:b + 1] if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == B else v

    return (mix[b], lt[b:b + 1], item(track_dict), lf[b:b + 1], item(fx_dict), lm[b:b + 1], item(master_dict),
            {name: h[:, b].tolist() for name, h in loss_history.items()})


def best_of(result):
    """The item of an ``optimize_batch(..., keep_best=True)`` result with the lowest ``best_loss`` (the first of equals), in
    ``optimize``'s 8-tuple form: ``pick(result, argmin)``."""
    if len(result) != 10 or not isinstance(result[9], FitReport):
        raise ValueError("best_of takes the result of optimize_batch(..., keep_best=True)")
    report = result[9]
    ranked = [(loss, b) for b, (loss, at) in enumerate(zip(report.best_loss, report.best_iteration)) if at is not None]
    if not ranked:
        raise ValueError("no item has a best iterate")
    return pick(result, min(ranked)[1])


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
