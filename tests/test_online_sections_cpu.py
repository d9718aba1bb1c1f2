"""``mst.online.optimize_sections`` / ``take_sections`` and ``AudioFeatureLoss.pooled`` without a GPU: the alias package and
``diffmst_hip`` export them, and what is wrong with the types and shapes of a call is said before anything touches a device (host
tensors are refused only after that)."""
import pytest
import torch


class Pooled:
    def pooled(self, mix, target):
        raise AssertionError("the loss was called")


def test_alias_and_package_export_the_sectioned_fit():
    import diffmst_hip
    import mst.loss
    import mst.online

    assert mst.online is diffmst_hip.online
    assert callable(mst.online.optimize_sections) and callable(mst.online.take_sections)
    assert callable(mst.loss.AudioFeatureLoss.pooled)  # what install() rebinds mst.loss.AudioFeatureLoss to carries it
    assert diffmst_hip._TARGETS[2][2] is diffmst_hip.loss.AudioFeatureLoss and len(diffmst_hip._TARGETS) == 5
    from mst import _cabi

    for name in ("mst_logit_adam_init_sections", "mst_logit_adam_step_sections", "mst_af_profile_pooled",
                 "mst_afloss_forward_profile_pooled", "mst_afloss_backward_profile_pooled"):
        assert name in _cabi.SIGNATURES
    assert _cabi.ABI_VERSION == 13 and _cabi.OPT_MAX_SECTIONS == 64


def test_take_sections():
    from mst.online import take_sections

    tracks = torch.arange(3 * 100.0).reshape(3, 100)
    got = take_sections(tracks, (0, 60, 10), 40)
    assert tuple(got.shape) == (3, 3, 40) and got.is_contiguous()
    for s, start in enumerate((0, 60, 10)):
        assert torch.equal(got[s], tracks[:, start:start + 40])
    for starts, length in (((), 40), ((0,), 0), ((-1,), 40), ((61,), 40)):
        with pytest.raises(ValueError):
            take_sections(tracks, starts, length)
    with pytest.raises(ValueError):
        take_sections(tracks[0], (0,), 40)


def test_type_and_shape_errors_come_before_any_device_call():
    from mst.loss import AudioFeatureLoss, AudioFeatureProfile
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_sections

    console, loss = AdvancedMixConsole(44100), Pooled()
    tracks, ref = torch.zeros(3, 2, 32768), torch.zeros(2, 32768)
    with pytest.raises(TypeError, match="pooled"):
        optimize_sections(tracks, ref, console, lambda a, b: None)
    with pytest.raises(TypeError, match="AudioFeatureProfile"):
        optimize_sections(tracks, ref.numpy(), console, loss)
    for bad_tracks in (tracks[0], tracks[0, 0], torch.zeros(65, 1, 8), torch.zeros(0, 2, 8)):
        with pytest.raises(ValueError):
            optimize_sections(bad_tracks, ref, console, loss)
    for bad_ref in (ref[:1], ref[0], torch.zeros(3, 3, 32768)):
        with pytest.raises(ValueError, match="ref_mix"):
            optimize_sections(tracks, bad_ref, console, loss)
    with pytest.raises(ValueError, match="batch size 1"):
        optimize_sections(tracks, AudioFeatureProfile(torch.zeros(2, 54, dtype=torch.float64), 44100), console, loss)
    with pytest.raises(ValueError, match="patience"):
        optimize_sections(tracks, ref, console, loss, patience=3)
    # well-formed host tensors get as far as the device check, like optimize()
    for good_ref in (ref, torch.zeros(2, 2, 20000), AudioFeatureProfile(torch.zeros(1, 54, dtype=torch.float64), 44100)):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            optimize_sections(tracks, good_ref, console, loss, n_iters=1)
    real = AudioFeatureLoss([1.0] * 5, 44100)
    with pytest.raises(TypeError, match="AudioFeatureProfile"):
        real.pooled(tracks, "a target")
    with pytest.raises(RuntimeError, match="CPU tensor"):
        real.pooled(tracks, AudioFeatureProfile(torch.zeros(1, 54, dtype=torch.float64), 44100))
