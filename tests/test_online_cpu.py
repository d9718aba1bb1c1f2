"""``mst.online`` without a GPU: the start point of ``optimize`` is the three host draws of the reference's scripts/online.py:39-45, in
its order and with its shapes; the stand-alone alias exports the module; CPU tensors are refused before anything else happens."""
import pytest
import torch


def script_draws(n_tracks, init_scale, generator=None):
    """The script's lines, restated: tracks, fx bus, master bus."""
    track_params = init_scale * torch.randn(n_tracks, 27, generator=generator)
    fx_bus_params = init_scale * torch.randn(1, 25, generator=generator)
    master_bus_params = init_scale * torch.randn(1, 26, generator=generator)
    return track_params, fx_bus_params, master_bus_params


@pytest.mark.parametrize("n_tracks,init_scale", [(1, 0.001), (16, 0.5)])
def test_start_point_is_the_scripts(n_tracks, init_scale):
    from mst.modules import AdvancedMixConsole
    from mst.online import start_point

    console = AdvancedMixConsole(44100)
    torch.manual_seed(11)
    got = start_point(n_tracks, console, init_scale)
    torch.manual_seed(11)
    want = script_draws(n_tracks, init_scale)
    assert [tuple(t.shape) for t in got] == [(n_tracks, 27), (1, 25), (1, 26)]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    state = torch.get_rng_state()
    got = start_point(n_tracks, console, init_scale, generator=torch.Generator().manual_seed(5))
    want = script_draws(n_tracks, init_scale, torch.Generator().manual_seed(5))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(torch.get_rng_state(), state)  # a generator of one's own leaves the global one alone


def test_alias_exports_the_module():
    import diffmst_hip
    import mst
    import mst.online

    assert mst.online is diffmst_hip.online
    assert callable(mst.online.optimize) and callable(mst.online.render_blocks)


def test_cpu_tensors_are_refused():
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize, render_blocks

    console = AdvancedMixConsole(44100)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        optimize(torch.zeros(2, 32768), torch.zeros(2, 32768), console, lambda a, b: None, n_iters=1)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        render_blocks(torch.zeros(2, 32768), torch.zeros(1, 2, 27), torch.zeros(1, 25), torch.zeros(1, 26), console)
