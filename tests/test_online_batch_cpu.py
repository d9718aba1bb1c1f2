"""``mst.online.optimize_batch`` / ``pick`` without a GPU: the alias package and ``diffmst_hip`` export them, and what is wrong with the
types and shapes of a call is said before anything touches a device (host tensors are refused only after that)."""
import pytest
import torch


class PerItem:
    def per_item(self, mix, target):
        raise AssertionError("the loss was called")


def test_alias_and_package_export_the_batched_fit():
    import diffmst_hip
    import mst.loss
    import mst.online

    assert mst.online is diffmst_hip.online
    assert callable(mst.online.optimize_batch) and callable(mst.online.pick)
    assert callable(mst.loss.AudioFeatureLoss.per_item)  # what install() rebinds mst.loss.AudioFeatureLoss to carries it
    assert diffmst_hip._TARGETS[2][2] is diffmst_hip.loss.AudioFeatureLoss
    from mst import _cabi

    for name in ("mst_logit_adam_batch_state_bytes", "mst_logit_adam_init_batch", "mst_logit_adam_step_batch",
                 "mst_afloss_forward_profile_items", "mst_afloss_backward_profile_items"):
        assert name in _cabi.SIGNATURES


def test_type_and_shape_errors_come_before_any_device_call():
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_batch

    console, loss = AdvancedMixConsole(44100), PerItem()
    tracks, ref = torch.zeros(3, 2, 32768), torch.zeros(3, 2, 32768)
    with pytest.raises(TypeError, match="per_item"):
        optimize_batch(tracks, ref, console, lambda a, b: None)
    with pytest.raises(TypeError, match="AudioFeatureProfile"):
        optimize_batch(tracks, ref.numpy(), console, loss)
    for bad_tracks, kw in ((tracks[0], {}), (tracks[0, 0], dict(batch=2)), (tracks, dict(batch=2)), (tracks[0], dict(batch=0)),
                           (tracks[0], dict(batch=1025))):
        with pytest.raises(ValueError):
            optimize_batch(bad_tracks, ref, console, loss, **kw)
    for bad_ref in (ref[:2], ref[:, :1], ref[0, 0], torch.zeros(3, 32768)):
        with pytest.raises(ValueError, match="ref_mix"):
            optimize_batch(tracks, bad_ref, console, loss)
    from mst.loss import AudioFeatureProfile

    with pytest.raises(ValueError, match="batch size 3 or 1"):
        optimize_batch(tracks, AudioFeatureProfile(torch.zeros(2, 54, dtype=torch.float64), 44100), console, loss)
    with pytest.raises(ValueError, match="init_scale"):
        optimize_batch(tracks, ref, console, loss, init_scale=[0.1, 0.2])
    # well-formed host tensors get as far as the device check, like optimize()
    for good_ref in (ref, ref[0], AudioFeatureProfile(torch.zeros(1, 54, dtype=torch.float64), 44100)):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            optimize_batch(tracks, good_ref, console, loss, init_scale=[0.1, 0.2, 0.3], n_iters=1)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        optimize_batch(tracks[0], ref[0], console, loss, batch=4, n_iters=1)


def test_pick_returns_the_form_of_optimize():
    from mst.online import pick

    B, T, N = 3, 2, 8
    dicts = [{"fx": {"gain": torch.arange(float(B * k)).reshape(B, k)}} for k in (T, 1, 1)]
    history = {"loss": torch.arange(12.0).reshape(4, B), "rms": torch.ones(4, B)}
    result = (torch.arange(float(B * 2 * N)).reshape(B, 2, N), torch.zeros(B, T, 27), dicts[0], torch.zeros(B, 25), dicts[1],
              torch.ones(B, 26), dicts[2], history, [None, 2, None])
    out = pick(result, 1)
    assert len(out) == 8
    assert torch.equal(out[0], result[0][1]) and [tuple(out[i].shape) for i in (1, 3, 5)] == [(1, T, 27), (1, 25), (1, 26)]
    assert torch.equal(out[2]["fx"]["gain"], dicts[0]["fx"]["gain"][1:2]) and tuple(out[6]["fx"]["gain"].shape) == (1, 1)
    assert out[7] == {"loss": [1.0, 4.0, 7.0, 10.0], "rms": [1.0] * 4}
    assert torch.equal(pick(result, -1)[0], result[0][2])
    with pytest.raises(IndexError):
        pick(result, 3)
