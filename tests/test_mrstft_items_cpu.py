"""``MultiResolutionSTFTLoss.per_item`` / ``pooled`` and the fits on them without a GPU: the entry points are declared and bound, the
signatures are what ``mst.online`` asks of a loss, and what is wrong with a call is said before anything touches a device."""
import inspect

import pytest
import torch

R3 = dict(fft_sizes=[512, 2048, 8192], hop_sizes=[256, 1024, 4096], win_lengths=[512, 2048, 8192])


def make_loss(**kw):
    from mst.loss import MultiResolutionSTFTLoss

    return MultiResolutionSTFTLoss(**R3, **kw)


def test_the_entry_points_are_declared_and_bound():
    import os

    from mst import _cabi

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffmst_hip.h")).read()
    for name in ("mst_mrstft_forward_items", "mst_mrstft_forward_items_eval", "mst_mrstft_backward_items"):
        assert name in _cabi.SIGNATURES and f"int {name}(const mst_mrstft_desc* d, int32_t items," in header
    # additive: the version the earlier fits were added at
    assert _cabi.ABI_VERSION == 13


def test_the_signatures_are_what_the_fits_ask_for():
    from mst.loss import MultiResolutionSTFTLoss
    from mst.online import _takes_items

    per_item, pooled = (inspect.signature(getattr(MultiResolutionSTFTLoss, name)).parameters for name in ("per_item", "pooled"))
    assert list(per_item)[1:] == ["input", "target", "items"] and per_item["items"].default is None
    assert list(pooled)[1:] == ["input", "target", "items"] and pooled["items"].default == 1
    loss = make_loss()
    assert _takes_items(loss.pooled) and callable(loss.per_item) and not hasattr(loss, "profile") and loss.paired


def test_per_item_refusals_come_before_any_device_call():
    x, y = torch.zeros(4, 2, 16384), torch.zeros(4, 2, 16384)
    for sync in (True, object()):
        for call in (make_loss(sync_group=sync).per_item, make_loss(sync_group=sync, sc_per_example=False).pooled):
            with pytest.raises(ValueError, match="sync_group"):
                call(x, y)
    loss = make_loss()
    with pytest.raises(NotImplementedError, match="target's gradient"):
        loss.per_item(x, y.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="target's gradient"):
        loss.pooled(x, y.clone().requires_grad_(True))
    for bad in (3, 0, -1, 1.5, True, 8):
        with pytest.raises(ValueError, match="items"):
            loss.per_item(x, y, items=bad)
    with pytest.raises(ValueError, match="differ"):
        loss.per_item(x, y[:2])
    with pytest.raises(TypeError):
        loss.per_item(x, "a target")
    # well-formed host tensors get as far as the device check
    for call, kw in ((loss.per_item, {}), (loss.per_item, dict(items=2)), (loss.pooled, {}), (loss.pooled, dict(items=4))):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            call(x, y, **kw)
    with torch.no_grad(), pytest.raises(RuntimeError, match="CPU tensor"):
        loss.per_item(x, y.clone().requires_grad_(True))  # nothing is differentiated: nothing to refuse


def test_a_sectioned_paired_reference_must_be_cut_like_the_tracks():
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_sections, optimize_sections_batch, take_sections

    console, loss = AdvancedMixConsole(44100), make_loss()
    n, S, B, T = 16384, 3, 2, 2
    tracks = torch.zeros(S, T, n)
    for bad in (torch.zeros(2, n), torch.zeros(S - 1, 2, n), torch.zeros(S + 1, 2, n), torch.zeros(S, 2, n - 1), torch.zeros(S, 2, 2 * n),
                torch.zeros(S, 1, n), torch.zeros(1, S, 2, n)):
        with pytest.raises(ValueError, match="MultiResolutionSTFTLoss is a paired loss.*cut like the tracks"):
            optimize_sections(tracks, bad, console, loss, n_iters=1)
    batch = torch.zeros(B, S, T, n)
    for bad in (torch.zeros(2, n), torch.zeros(B, 2, n), torch.zeros(S + 1, 2, n), torch.zeros(B, S - 1, 2, n), torch.zeros(B + 1, S, 2, n),
                torch.zeros(B, S, 2, n + 1), torch.zeros(S, 2, n // 2)):
        with pytest.raises(ValueError, match="MultiResolutionSTFTLoss is a paired loss.*cut like the tracks"):
            optimize_sections_batch(batch, bad, console, loss, n_iters=1)
        with pytest.raises(ValueError, match="paired loss"):
            optimize_sections_batch(tracks, bad, console, loss, n_iters=1, batch=B)
    # the accepted forms get as far as the device check; take_sections cuts a (2, N) reference like the tracks
    song, ref = torch.zeros(T, 3 * n), torch.zeros(2, 3 * n)
    starts = (0, 5000, 2 * n)
    cut, ref_cut = take_sections(song, starts, n), take_sections(ref, starts, n)
    assert cut.shape == (S, T, n) and ref_cut.shape == (S, 2, n) and ref_cut.is_contiguous()
    with pytest.raises(RuntimeError, match="CPU tensor"):
        optimize_sections(cut, ref_cut, console, loss, n_iters=1)
    for good_tracks, good_ref, kw in ((batch, ref_cut, {}), (batch, torch.zeros(B, S, 2, n), {}), (cut, ref_cut, dict(batch=B))):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            optimize_sections_batch(good_tracks, good_ref, console, loss, n_iters=1, **kw)


def test_a_batch_takes_the_paired_reference_forms():
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_batch

    console, loss = AdvancedMixConsole(44100), make_loss()
    tracks = torch.zeros(3, 2, 16384)
    for bad in (torch.zeros(2, 2, 16384), torch.zeros(3, 1, 16384), torch.zeros(16384)):
        with pytest.raises(ValueError, match="ref_mix"):
            optimize_batch(tracks, bad, console, loss, n_iters=1)
    for good in (torch.zeros(2, 16384), torch.zeros(3, 2, 16384)):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            optimize_batch(tracks, good, console, loss, n_iters=1)


def test_what_needs_a_profile_is_refused_as_the_missing_method():
    """A stored profile, or (in a batch) a reference of another length, can only be fitted with a loss that has ``profile``: a paired
    loss is refused with the TypeError of a missing method, naming the method the fit would have called, before any device call."""
    from mst.loss import AudioFeatureProfile
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_batch, optimize_sections, optimize_sections_batch

    console, loss = AdvancedMixConsole(44100), make_loss()
    profile = lambda bs: AudioFeatureProfile(torch.zeros(bs, 54, dtype=torch.float64), 44100)
    tracks = torch.zeros(3, 2, 16384)
    for ref in (torch.zeros(3, 2, 20000), torch.zeros(2, 8192), profile(3), profile(1)):
        with pytest.raises(TypeError, match="per_item is paired"):
            optimize_batch(tracks, ref, console, loss, n_iters=1)
    with pytest.raises(TypeError, match="pooled is paired.*AudioFeatureProfile"):
        optimize_sections(tracks, profile(1), console, loss, n_iters=1)
    for ref in (profile(1), profile(2)):
        with pytest.raises(TypeError, match="pooled is paired.*AudioFeatureProfile"):
            optimize_sections_batch(torch.zeros(2, 3, 2, 16384), ref, console, loss, n_iters=1)
