"""The console must not depend on what its workspace holds when it arrives: the product allocates it with ``torch.empty``.  At a length
whose 64-sample chunk count is no multiple of 256 (17000 samples: 266 chunks, padded to 512) the backward reads the padding of the
all-pole chunk start states and multiplies it by zero samples, so a NaN left there by whoever owned the memory before came out as NaN
in every track and master gradient.  On the host simulator: a NaN-filled workspace gives the bits of a zero-filled one."""
import torch


def test_console_gradients_do_not_depend_on_the_workspace_contents(monkeypatch):
    from hostsim import harness
    from mst.modules import AdvancedMixConsole

    T, n = 2, 17000
    g = torch.Generator().manual_seed(0)
    tracks = 0.1 * torch.randn(1, T, n, generator=g)
    tp, fp, mp = (0.25 + 0.5 * torch.rand(shape, generator=g) for shape in ((1, T, 27), (1, 25), (1, 26)))
    grad_mix = torch.randn(1, 2, n, generator=g)
    flags = dict(use_track_input_fader=True, use_track_eq=True, use_track_compressor=True, use_track_panner=True, use_fx_bus=False,
                 use_master_bus=True, use_output_fader=True)
    ranges = AdvancedMixConsole(44100).param_ranges
    workspace = harness._workspace
    outs = []
    for fill in (0.0, float("nan")):
        monkeypatch.setattr(harness, "_workspace", lambda nbytes, _fill, fill=fill: workspace(nbytes, fill))
        outs.append(harness.console(ranges, tracks, tp, fp, mp, flags, grad_mix=grad_mix, want_mixed=False))
    clean, dirty = outs
    assert clean["status"] == dirty["status"] == 0
    for key in ("mix", "grad_tp", "grad_mp"):
        assert bool(torch.isfinite(dirty[key]).all()), f"{key}: not finite from a NaN-filled workspace"
        assert torch.equal(clean[key].view(torch.int32), dirty[key].view(torch.int32)), f"{key} depends on the workspace contents"
    assert bool((clean["grad_tp"] != 0).any()) and bool((clean["grad_mp"] != 0).any())
