"""``mst.utils.windowed_loudness`` and ``mst.online.pick_sections`` without a GPU: the alias package and ``diffmst_hip`` export them,
the window arithmetic is right, and what is wrong with a call is said before anything touches a device (host tensors are refused only
after that)."""
import pytest
import torch

import loudness_ref as R
import loudness_windows_ref as WR


def test_alias_and_package_export_the_picker():
    import diffmst_hip
    import mst.online
    import mst.utils
    from mst import _cabi

    assert mst.online is diffmst_hip.online and mst.utils is diffmst_hip.utils
    assert callable(mst.utils.windowed_loudness) and callable(mst.online.pick_sections)
    assert mst.online.SectionPick._fields == ("starts", "length", "active", "covered", "track_lufs", "mix_lufs")
    for name in ("mst_loudness_num_windows", "mst_loudness_windows_workspace_bytes", "mst_loudness_windows", "mst_pick_sections"):
        assert name in _cabi.SIGNATURES
    assert _cabi.ABI_VERSION == 13 and len(diffmst_hip._TARGETS) == 5
    assert (_cabi.OPT_MAX_SECTIONS, _cabi.LOUDNESS_MAX_BLOCKS, _cabi.PICK_MAX_TRACKS) == (64, 4092, 256)


def test_header_names_the_limits():
    import os
    import re

    from mst import _cabi

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffmst_hip.h")).read()
    for name, value in (("MST_OPT_MAX_SECTIONS", _cabi.OPT_MAX_SECTIONS), ("MST_LOUDNESS_MAX_BLOCKS", _cabi.LOUDNESS_MAX_BLOCKS),
                        ("MST_PICK_MAX_TRACKS", _cabi.PICK_MAX_TRACKS)):
        assert re.search(rf"#define {name} {value}\b", header), name


@pytest.mark.parametrize("rate", [44100, 48000, 22050, 32000, 96000, 88200, 24000])
def test_window_arithmetic(rate):
    from mst.utils import loudness_window_grid

    step = rate // 10
    n = 30 * step + 17           # 27 complete blocks
    assert WR.num_complete_blocks(n, rate) == 27
    for length, hop, W, H in ((4 * step, None, 1, 1), (5 * step - 1, None, 1, 1), (5 * step, 2 * step, 2, 2), (131072, 3 * step, 131072 // step - 3, 3),
                              (30 * step, None, 27, 1)):
        if length > n:
            continue
        got_w, got_h, starts = loudness_window_grid(n, length, hop, rate)
        assert (got_w, got_h) == (W, H) and len(starts) == WR.num_windows(27, W, H)
        assert got_w == (10 * length - 4 * rate) // rate + 1  # floor((length - 0.4 rate) / (0.1 rate)) + 1 in integers
        for w, start in enumerate(starts):
            assert start == R.block_bounds(w * H, rate)[0] == w * H * step
            assert R.block_bounds(w * H + W - 1, rate)[1] <= min(n, start + length)  # the window's blocks lie inside it
    assert loudness_window_grid(4 * step, 4 * step, None, rate) == (1, 1, [0])


def test_grid_errors():
    from mst.utils import loudness_window_grid

    for args in ((70000, 17639), (70000, 17640, 0), (70000, 17640, 4411), (70000, 17640, -4410), (70000, 17640, 2205.0), (17639, 17640),
                 (70000, 13 * 4410 + 17640), (17640 + 4092 * 4410, 17640), (70000, 17640, None, 44101), (70000, 17640, None, 8000),
                 (70000, 17640, None, 44100.5)):
        with pytest.raises(ValueError):
            loudness_window_grid(*args)
    assert len(loudness_window_grid(17640 + 4091 * 4410, 17640)[2]) == 4092


def test_errors_come_before_any_device_call():
    from mst.online import pick_sections
    from mst.utils import windowed_loudness

    tracks = torch.zeros(3, 70000)
    with pytest.raises(TypeError):
        pick_sections(tracks.numpy(), 30000, 2)
    for bad in (dict(length=30000.0), dict(count=2.0), dict(count=True)):
        with pytest.raises(TypeError):
            pick_sections(tracks, **{"length": 30000, "count": 2, **bad})
    for bad_tracks in (tracks[0], tracks[None], tracks.long(), torch.zeros(257, 70000), torch.zeros(0, 70000)):
        with pytest.raises(ValueError):
            pick_sections(bad_tracks, 30000, 2)
    for kw in (dict(count=0), dict(count=65), dict(length=17639), dict(length=70001), dict(hop=1000), dict(sample_rate=44101),
               dict(min_gap=-1), dict(min_gap=0.5), dict(track_floor_lufs=torch.zeros(2)), dict(track_floor_lufs=torch.zeros(3, 1))):
        with pytest.raises(ValueError):
            pick_sections(tracks, **{"length": 30000, "count": 2, **kw})
    with pytest.raises(ValueError):
        pick_sections(tracks, 30000, 2, track_floor_lufs="loud")
    # well-formed host tensors get as far as the device check
    for kw in (dict(), dict(track_floor_lufs=torch.full((3,), -40.0), min_gap=0, hop=8820)):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            pick_sections(tracks, 30000, 2, **kw)
    for bad in ((torch.zeros(70000), 30000), (torch.zeros(6, 70000), 30000), (tracks, 17639), (tracks, 30000, 100), (tracks, 30000, None, 44101)):
        with pytest.raises(ValueError):
            windowed_loudness(*bad)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        windowed_loudness(tracks, 30000)
