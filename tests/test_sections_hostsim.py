"""``mst_pick_sections`` (diff-mst_amd/csrc/mst_sections.hip) on the host simulator against the numpy restatement of its rule
(tests/sections_ref.py): exact equality of all three outputs, on random tables and on hand-worked cases, and its limits."""
import numpy as np
import pytest
import torch

import sections_ref as S

NINF, NAN = float("-inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from hostsim import harness

    return harness.lib()


def both(lib, track, mix, floor, mix_floor, count, gap):
    track, mix, floor = (np.asarray(v, np.float32) for v in (track, mix, floor))
    want = S.pick_sections(track, mix, floor, mix_floor, count, gap)
    got = S.call_picker(lib, torch.from_numpy(track), torch.from_numpy(mix), torch.from_numpy(floor), mix_floor, count, gap)
    for g, w, name in zip(got, want, ("windows", "active", "covered")):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{name}: {g} != {w}"
    return got


@pytest.mark.parametrize("T,NW,count,gap", [(1, 1, 1, 1), (16, 5, 8, 1), (3, 257, 4, 30), (256, 4092, 64, 7)])
def test_random_tables(lib, T, NW, count, gap):
    track, mix, floor, mix_floor = S.random_tables(T, NW, 100 + T)
    if (T, NW) == (1, 1):
        track[0, 0], mix[0] = -20.0, -10.0  # the one window there is can be taken
    windows, active, covered = both(lib, track, mix, floor, mix_floor, count, gap)
    taken = windows[windows >= 0]
    print(f"\n[{T} tracks, {NW} windows] {len(taken)} of {count} taken, {int(covered.sum())} tracks covered")
    assert len(set(taken.tolist())) == len(taken)
    assert len(taken) >= min(2, NW) and covered.any()  # the tables are not degenerate


def test_cover_beats_the_louder_mix(lib):
    # tracks 0 and 1 are each active in one window only; window 2 has the louder mix and track 2, which plays everywhere
    track = [[-20, NINF, NINF, NINF], [NINF, NINF, NINF, -20], [-30, -30, -20, -30]]
    windows, active, covered = both(lib, track, [-25, -25, -10, -25], [-48] * 3, -48.0, 2, 1)
    assert windows.tolist() == [0, 3] and covered.tolist() == [1, 1, 1]
    assert active.tolist() == [[1, 0, 1], [0, 1, 1]]
    # with a third section the louder window follows
    assert both(lib, track, [-25, -25, -10, -25], [-48] * 3, -48.0, 3, 1)[0].tolist() == [0, 3, 2]


def test_a_tie_falls_to_the_lower_index(lib):
    track = [[-20, -20, -20, -20]]
    assert both(lib, track, [-15, -12, -12, -15], [-48], -48.0, 4, 1)[0].tolist() == [1, 2, 0, 3]
    assert both(lib, track, [-0.0, 0.0, 0.0, -0.0], [-48], -48.0, 2, 1)[0].tolist() == [0, 1]  # -0 and +0 are one loudness


def test_min_gap_excludes_a_neighbour(lib):
    track = [[-20] * 6]
    mix = [-30, -10, -11, -12, -30, -13]
    assert both(lib, track, mix, [-48], -48.0, 3, 1)[0].tolist() == [1, 2, 3]
    assert both(lib, track, mix, [-48], -48.0, 3, 2)[0].tolist() == [1, 3, 5]
    assert both(lib, track, mix, [-48], -48.0, 3, 3)[0].tolist() == [1, 5, -1]


def test_fewer_candidates_than_count(lib):
    track = [[-20, -60, -20], [-60, -60, -20]]
    windows, active, covered = both(lib, track, [-20, -20, -50], [-48, -48], -48.0, 4, 1)
    assert windows.tolist() == [0, -1, -1, -1] and covered.tolist() == [1, 0]  # window 1: nobody plays; window 2: the mix is too quiet
    assert active.tolist() == [[1, 0], [0, 0], [0, 0], [0, 0]]


def test_nothing_eligible(lib):
    windows, active, covered = both(lib, [[-60, -70], [NINF, -49]], [-10, -10], [-48, -48], -48.0, 3, 1)
    assert windows.tolist() == [-1, -1, -1] and not active.any() and not covered.any()
    assert both(lib, [[-20, -20]], [-10, -10], [-48], NAN, 2, 1)[0].tolist() == [-1, -1]


def test_nan_and_silence_are_inactive(lib):
    track = [[NAN, -20, NINF], [NINF, NAN, -20], [NAN, NAN, NINF]]
    windows, active, covered = both(lib, track, [-5, NAN, -30], [-48, -48, NINF], NINF, 3, 1)
    # window 0: nobody; window 1: a NaN mix; window 2: track 1 - and track 2 too, whose floor of -inf its -inf reaches
    assert windows.tolist() == [2, -1, -1] and covered.tolist() == [0, 1, 1] and active[0].tolist() == [0, 1, 1]


def test_limits_are_a_status(lib):
    from mst import _cabi

    def call(T, NW, count, gap, drop=None):
        args = dict(track=torch.zeros(max(T, 1), max(NW, 1)), mix=torch.zeros(max(NW, 1)), floor=torch.zeros(max(T, 1)),
                    windows=torch.zeros(max(count, 1), dtype=torch.int32), active=torch.zeros(max(count, 1) * max(T, 1), dtype=torch.uint8),
                    covered=torch.zeros(max(T, 1), dtype=torch.uint8))
        if drop:
            args[drop] = None
        lib.mst_pick_sections(args["track"], args["mix"], args["floor"], -48.0, T, NW, count, gap, args["windows"], args["active"],
                              args["covered"], None)

    call(2, 3, 2, 1)
    assert (_cabi.PICK_MAX_TRACKS, _cabi.LOUDNESS_MAX_BLOCKS, _cabi.OPT_MAX_SECTIONS) == (256, 4092, 64)
    for bad in ((0, 3, 2, 1), (257, 3, 2, 1), (2, 0, 2, 1), (2, 4093, 2, 1), (2, 3, 0, 1), (2, 3, 65, 1), (2, 3, 2, 0)):
        with pytest.raises(_cabi.AbiError) as e:
            call(*bad)
        assert e.value.code != 0
    for name in ("track", "mix", "floor", "windows", "active", "covered"):
        with pytest.raises(_cabi.AbiError):
            call(2, 3, 2, 1, drop=name)
