"""``mst.online.optimize_sections_batch`` and ``AudioFeatureLoss.pooled(..., items=B)`` without a GPU: the alias package and
``diffmst_hip`` export them, ``install()`` / ``uninstall()`` expose and remove the name with the ``mst.online`` alias, and what is wrong
with the types and shapes of a call is said before anything touches a device (host tensors are refused only after that)."""
import sys
import types

import pytest
import torch


class Pooled:
    def pooled(self, mix, target, items=1):
        raise AssertionError("the loss was called")


class PooledWithoutItems:
    def pooled(self, mix, target):
        raise AssertionError("the loss was called")


def test_alias_and_package_export_the_batched_sectioned_fit():
    import diffmst_hip
    import mst.online
    from mst import _cabi

    assert mst.online is diffmst_hip.online and callable(mst.online.optimize_sections_batch)
    for name in ("mst_logit_adam_init_sections_batch", "mst_logit_adam_step_sections_batch"):
        assert name in _cabi.SIGNATURES
    assert _cabi.ABI_VERSION == 13 and _cabi.OPT_MAX_SECTIONS == 64 and _cabi.OPT_MAX_ITEMS == 1024


def test_install_exposes_and_uninstall_removes_the_name(monkeypatch):
    import diffmst_hip

    import inspect

    # stand-ins for the reference's modules (the alias package must not be what install() finds): its own names, to be swapped and restored
    theirs = {}
    fake = types.ModuleType("mst")
    fake.__path__ = []
    monkeypatch.setitem(sys.modules, "mst", fake)
    for modname, attr, _ in diffmst_hip._TARGETS:
        module = types.ModuleType(modname)
        theirs[modname, attr] = type(attr, (), {})
        setattr(module, attr, theirs[modname, attr])
        monkeypatch.setitem(sys.modules, modname, module)
    monkeypatch.setitem(sys.modules, "auraloss", types.ModuleType("auraloss"))
    assert not diffmst_hip._installed
    swapped = diffmst_hip.install()
    try:
        assert len(swapped) == 5
        cls = sys.modules["mst.loss"].AudioFeatureLoss
        assert cls is diffmst_hip.loss.AudioFeatureLoss
        assert "items" in inspect.signature(cls.pooled).parameters and "items" in inspect.signature(cls.profile).parameters
        assert diffmst_hip.online._takes_items(cls([1.0] * 5, 44100).pooled)  # what optimize_sections_batch asks of a loss
    finally:
        diffmst_hip.uninstall()
    assert not diffmst_hip._installed
    for (modname, attr), old in theirs.items():
        assert getattr(sys.modules[modname], attr) is old


def test_type_and_shape_errors_come_before_any_device_call():
    from mst.loss import AudioFeatureProfile
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_sections_batch

    console, loss = AdvancedMixConsole(44100), Pooled()
    tracks, ref = torch.zeros(2, 3, 2, 32768), torch.zeros(2, 32768)  # B = 2, S = 3, T = 2
    profile = lambda bs: AudioFeatureProfile(torch.zeros(bs, 54, dtype=torch.float64), 44100)
    # a loss without pooled, or whose pooled takes no items
    for bad_loss in (lambda a, b: None, PooledWithoutItems()):
        with pytest.raises(TypeError, match="pooled"):
            optimize_sections_batch(tracks, ref, console, bad_loss)
    with pytest.raises(TypeError, match="AudioFeatureProfile"):
        optimize_sections_batch(tracks, ref.numpy(), console, loss)
    # tracks with wrong dimensions, batch disagreeing with tracks, B or S outside their limits
    for bad_tracks, batch in ((tracks[0, 0], None), (tracks[0, 0, 0], None), (tracks[None], None), (tracks[0], None), (tracks, 3),
                              (tracks[0], 0), (tracks[0], 1025), (torch.zeros(2, 65, 1, 8), None), (torch.zeros(2, 0, 1, 8), None),
                              (torch.zeros(0, 2, 1, 8), None), (torch.zeros(1025, 1, 1, 8), None), (torch.zeros(65, 1, 8), 2)):
        with pytest.raises(ValueError):
            optimize_sections_batch(bad_tracks, ref, console, loss, batch=batch)
    # every wrong ref_mix form
    for bad_ref in (ref[:1], ref[0], torch.zeros(3, 2, 32768), torch.zeros(2, 3, 32768), torch.zeros(3, 4, 2, 32768),
                    torch.zeros(2, 4, 3, 32768), torch.zeros(2, 0, 2, 32768), torch.zeros(1, 2, 4, 2, 32768)):
        with pytest.raises(ValueError, match="ref_mix"):
            optimize_sections_batch(tracks, bad_ref, console, loss)
    with pytest.raises(ValueError, match="batch size 2 or 1"):
        optimize_sections_batch(tracks, profile(3), console, loss)
    # an init_scale sequence of the wrong length
    for bad_scale in ((0.001,), (0.001, 0.01, 0.1)):
        with pytest.raises(ValueError, match="init_scale"):
            optimize_sections_batch(tracks, ref, console, loss, init_scale=bad_scale)
    # the patience / poll_every rules of _check_best
    for bad in (dict(patience=3), dict(min_delta=0.1), dict(keep_best=True, patience=-1), dict(keep_best=True, poll_every=2),
                dict(keep_best=True, patience=2, poll_every=0), dict(keep_best=True, min_delta=-1.0),
                dict(keep_best=True, min_delta=float("nan"))):
        with pytest.raises(ValueError):
            optimize_sections_batch(tracks, ref, console, loss, **bad)
    # well-formed host tensors get as far as the device check, like optimize_batch()
    for good_tracks, good_ref, kw in ((tracks, ref, {}), (tracks, torch.zeros(2, 2, 20000), {}), (tracks, torch.zeros(2, 4, 2, 20000), {}),
                                      (tracks, profile(2), {}), (tracks, profile(1), {}), (tracks[0], profile(1), dict(batch=4)),
                                      (tracks, ref, dict(init_scale=(0.001, 0.01))), (tracks, ref, dict(batch=2)),
                                      (tracks, ref, dict(keep_best=True, patience=2, poll_every=2))):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            optimize_sections_batch(good_tracks, good_ref, console, loss, n_iters=1, **kw)


def test_pooled_and_profile_refuse_host_tensors_and_bad_targets():
    from mst.loss import AudioFeatureLoss, AudioFeatureProfile

    real = AudioFeatureLoss([1.0] * 5, 44100)
    x = torch.zeros(4, 2, 32768)
    with pytest.raises(TypeError, match="AudioFeatureProfile"):
        real.pooled(x, "a target", items=2)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        real.pooled(x, AudioFeatureProfile(torch.zeros(2, 54, dtype=torch.float64), 44100), items=2)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        real.profile(x, pool=True, items=2)
