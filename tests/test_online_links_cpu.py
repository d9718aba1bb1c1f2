"""Linked fits without a GPU: ``links_from_stereo_id``, the binding of the two new entry points, and every ``ValueError`` of the
``links`` / ``stereo_id`` / ``mirror_pan`` keywords of the four ``optimize*`` functions, raised before anything touches a device (the
tracks and references here are host tensors, which a well-formed call refuses only after that)."""
import ctypes
import types

import pytest
import torch


class Pooled:
    def pooled(self, mix, target, items=1):
        raise AssertionError("the loss was called")

    def per_item(self, mix, target):
        raise AssertionError("the loss was called")

    def __call__(self, mix, target):
        raise AssertionError("the loss was called")


def test_binding_exports_the_linked_calls():
    import mst.online
    from mst import _cabi, _desc

    for name in ("mst_logit_adam_init_linked", "mst_logit_adam_step_linked"):
        assert name in _cabi.SIGNATURES
    assert _cabi.ABI_VERSION == 13 and _cabi.OPT_MAX_LINK_ROWS == 256
    assert ctypes.sizeof(_cabi.LogitAdamLinks) == 16 + 256  # four int32 and the leader bytes: mst_logit_adam_links
    assert _desc.TRACK_INDEX.index(("stereo_panner", "pan")) == 25
    assert callable(mst.online.links_from_stereo_id)


def test_links_from_stereo_id():
    from mst.online import links_from_stereo_id

    assert links_from_stereo_id([1, 0, 0, 0]) == [0, 0, 2, 3]
    assert links_from_stereo_id([0, 0, 0]) == [0, 1, 2]
    assert links_from_stereo_id([]) == []
    assert links_from_stereo_id([1, 0, 1, 0]) == [0, 0, 2, 2]
    assert links_from_stereo_id([0, 1, 0, 1, 0]) == [0, 1, 1, 3, 3]
    assert links_from_stereo_id([0, 0, 1]) == [0, 1, 2]  # a flag on the last row has no partner: ignored
    assert links_from_stereo_id([1]) == [0]
    assert links_from_stereo_id([1, 1, 0]) == [0, 0, 2]  # the partner is skipped when the flags are walked: its own flag is not read
    assert links_from_stereo_id(torch.tensor([1, 0, 0, 1, 0])) == [0, 0, 2, 3, 3]
    assert links_from_stereo_id(torch.tensor([1.0, 0.0])) == [0, 0]
    with pytest.raises(ValueError, match="1-D"):
        links_from_stereo_id(torch.zeros(2, 2))


def calls():
    """The four functions with well-formed host arguments at T = 4: (function, tracks, ref_mix)."""
    from mst import online

    ref = torch.zeros(2, 20000)
    return [(online.optimize, torch.zeros(4, 17000), ref), (online.optimize_batch, torch.zeros(2, 4, 17000), ref),
            (online.optimize_sections, torch.zeros(2, 4, 17000), ref), (online.optimize_sections_batch, torch.zeros(2, 2, 4, 17000), ref)]


@pytest.mark.parametrize("which", range(4))
def test_link_errors_come_before_any_device_call(which):
    from mst.modules import AdvancedMixConsole

    fn, tracks, ref = calls()[which]
    console, loss = AdvancedMixConsole(44100), Pooled()
    with pytest.raises(ValueError, match="not both"):
        fn(tracks, ref, console, loss, links=[0, 0, 2, 3], stereo_id=[1, 0, 0, 0])
    # an invalid map: a wrong length, a leader that points forward, one that does not lead itself, a negative or fractional entry
    for bad in ([0, 0, 2], [0, 0, 2, 3, 4], [1, 1, 2, 3], [0, 2, 2, 3], [0, 0, 1, 3], [0, -1, 2, 3], [0, 0.5, 2, 3]):
        with pytest.raises(ValueError, match="links"):
            fn(tracks, ref, console, loss, links=bad)
    with pytest.raises(ValueError, match="stereo_id"):
        fn(tracks, ref, console, loss, stereo_id=[1, 0, 0])
    # mirror_pan: a group of more than two rows; a console without the 27 track parameters
    with pytest.raises(ValueError, match="two rows"):
        fn(tracks, ref, console, loss, links=[0, 0, 0, 3])
    # (this package's BasicMixConsole keeps the 27-column layout; a console like the reference's gain-and-pan one has two columns)
    basic = types.SimpleNamespace(num_track_control_params=2, num_fx_bus_control_params=25, num_master_bus_control_params=26)
    with pytest.raises(ValueError, match="mirror_pan"):
        fn(tracks, ref, basic, loss, stereo_id=[1, 0, 0, 0])
    # more than 256 tracks
    many = torch.zeros(tracks.shape[:-2] + (257, 8))
    with pytest.raises(ValueError, match="256"):
        fn(many, ref, console, loss, links=list(range(257)))
    # well-formed linked calls get as far as the device check, like the unlinked ones
    for kw in (dict(links=[0, 0, 2, 3]), dict(stereo_id=[1, 0, 1, 0]), dict(stereo_id=torch.tensor([1, 0, 0, 1])),
               dict(links=[0, 0, 0, 3], mirror_pan=False), dict(links=[0, 1, 2, 3]), dict(stereo_id=[1, 0, 0, 0], keep_best=True)):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fn(tracks, ref, console, loss, n_iters=1, **kw)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        fn(tracks, ref, basic, loss, n_iters=1, stereo_id=[1, 0, 0, 0], mirror_pan=False)
