"""Host validation of the delivery meter's Python functions (diffmst_hip/utils.py: true_peak, short_term_loudness,
momentary_loudness, loudness_range, meter_report, loudness_normalize_limited): shapes, hop rules, rate rules and the forward-only
rule are all decided before anything touches a device, so none is needed here."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_functions_are_exported_through_mst_utils():
    import mst.utils as U

    for name in ("true_peak", "short_term_loudness", "momentary_loudness", "loudness_range", "meter_report", "LoudnessReport",
                 "loudness_normalize_limited", "short_term_grid", "true_peak_factor"):
        assert hasattr(U, name), name
    assert U.LoudnessReport._fields == ("integrated", "loudness_range", "momentary_max", "short_term_max", "true_peak", "sample_peak")


def test_tile_constant_is_the_headers():
    from mst import _cabi

    text = open(os.path.join(ROOT, "include", "diffmst_hip.h")).read()
    assert int(re.search(r"#define MST_TRUE_PEAK_TILE (\d+)", text).group(1)) == _cabi.TRUE_PEAK_TILE


def test_true_peak_rate_rules():
    import mst.utils as U

    assert [U.true_peak_factor(r) for r in (22050, 44100, 48000, 88200, 95999, 96000, 176400, 191999)] == [4, 4, 4, 4, 4, 2, 2, 2]
    for bad in (192000, 384000, 0, -44100, 44100.5, True):
        with pytest.raises(ValueError):
            U.true_peak_factor(bad)
    x = torch.zeros(2, 1000)
    with pytest.raises(ValueError, match="192000"):
        U.true_peak(x, 192000)
    with pytest.raises(ValueError):
        U.true_peak(torch.zeros(1000))          # no channel dimension
    with pytest.raises(ValueError, match="at least one sample"):
        U.true_peak(torch.zeros(2, 0))
    with pytest.raises(ValueError, match="65535"):
        U.true_peak(torch.zeros(32768, 2, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        U.true_peak(x)                          # a valid call gets as far as the device check: any length, any channel count
    with pytest.raises(RuntimeError, match="no CPU path"):
        U.true_peak(torch.zeros(3, 7, 1), 96000, per_channel=True)


def test_short_term_grid_hop_rules():
    import mst.utils as U

    n = 57 * 4410 + 100
    H, starts = U.short_term_grid(n)
    assert H == 10 and starts == [0, 44100, 88200]                      # default: one second; (57 - 30) // 10 + 1 windows
    H, starts = U.short_term_grid(n, hop=4410)
    assert H == 1 and len(starts) == 28 and starts[-1] == 27 * 4410
    assert U.short_term_grid(30 * 4800, hop=30 * 4800, sample_rate=48000) == (30, [0])
    for bad in (0, 4409, 4411, -4410, 31 * 4410, 4410.5, True):
        with pytest.raises(ValueError, match="hop"):
            U.short_term_grid(n, hop=bad)
    with pytest.raises(ValueError, match="3 s"):
        U.short_term_grid(30 * 4410 - 1)
    with pytest.raises(ValueError, match="rate / 10"):
        U.short_term_grid(n, sample_rate=44101)
    with pytest.raises(ValueError, match="4092"):
        U.short_term_grid(4096 * 4410)
    assert U.short_term_grid(4095 * 4410)[0] == 10


@pytest.mark.parametrize("name", ["short_term_loudness", "loudness_range", "meter_report"])
def test_range_functions_validate_on_the_host(name):
    import mst.utils as U

    fn = getattr(U, name)
    with pytest.raises(ValueError, match="3 s"):
        fn(torch.zeros(2, 100000))
    with pytest.raises(ValueError, match="five channels"):
        fn(torch.zeros(6, 200000))
    with pytest.raises(ValueError, match="rate / 10"):
        fn(torch.zeros(2, 200000), sample_rate=44101)
    if name != "meter_report":
        with pytest.raises(ValueError, match="hop"):
            fn(torch.zeros(2, 200000), hop=1000)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fn(torch.zeros(2, 200000))


def test_limited_normalisation_validates_on_the_host():
    import mst.utils as U

    with pytest.raises(ValueError, match="Audio must have length greater than the block size."):
        U.loudness_normalize_limited(torch.zeros(2, 17639), -14.0)
    with pytest.raises(ValueError, match="five channels"):
        U.loudness_normalize_limited(torch.zeros(6, 20000), -14.0)
    with pytest.raises(ValueError, match="192000"):
        U.loudness_normalize_limited(torch.zeros(2, 100000), -14.0, sample_rate=192000)
    with pytest.raises(RuntimeError, match="no CPU path"):
        U.loudness_normalize_limited(torch.zeros(2, 20000), -14.0)


def test_forward_only(monkeypatch):
    """With the device check out of the way the next thing a differentiable input meets is the forward-only rule - before the library."""
    import mst.utils as U

    monkeypatch.setattr(U._hip, "require_cuda", lambda *t: None)
    monkeypatch.setattr(U._hip, "lib", lambda: pytest.fail("the library was reached"))
    x = torch.zeros(2, 200000, requires_grad=True)
    calls = [lambda: U.true_peak(x), lambda: U.short_term_loudness(x), lambda: U.momentary_loudness(x), lambda: U.loudness_range(x),
             lambda: U.meter_report(x), lambda: U.loudness_normalize_limited(x, -14.0)]
    for call in calls:
        with pytest.raises(NotImplementedError, match="forward-only"):
            call()
