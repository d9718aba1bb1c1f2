"""``mst.utils.windowed_loudness`` and ``mst.online.pick_sections`` on the MI355X: the windows against the float64 restatement
(tests/loudness_windows_ref.py), against the meter on crops within the restatement's own warm-against-cold difference, the picker
kernel against its numpy restatement, and a synthetic song from ``pick_sections`` through ``take_sections`` into
``optimize_sections``.  Bounds and the gate-margin pre-check are those of tests/test_loudness_hostsim.py."""
import numpy as np
import pytest
import torch

import loudness_ref as R
import loudness_windows_ref as WR
import sections_ref as S

pytestmark = pytest.mark.gpu

FP32_ALLOWANCE_LU = 8.7e-5   # derived in tests/test_loudness_hostsim.py
GATE_MARGIN_LU = 1e-3


@pytest.mark.parametrize("rows,chs,n,rate,W,H,seed", [(16, 1, 262144, 44100, 11, 1, 201), (2, 2, 131072, 48000, 5, 2, 202)])
def test_windows_match_the_float64_restatement(rows, chs, n, rate, W, H, seed):
    from mst.utils import integrated_loudness, windowed_loudness

    step = rate // 10
    x = R.level_step_noise(rows, chs, n, seed)
    ref = [WR.windowed_loudness(x[r], rate, W, H) for r in range(rows)]
    seen_rel = seen_abs = seen_silent = False
    for r in range(rows):
        for w, (l, a, f) in enumerate(ref[r][1]):
            m_rel, m_abs = WR.window_margins(l)
            assert m_rel > GATE_MARGIN_LU and m_abs > GATE_MARGIN_LU, f"row {r} window {w}: a block sits on a gate, change the seed"
            seen_rel |= len(f) < len(a)
            seen_abs |= 0 < len(a) < W
            seen_silent |= not a
    assert seen_rel and seen_abs and seen_silent  # windows that lose blocks to each gate, and windows wholly in the 1e-6 stretch
    xd = torch.from_numpy(x).cuda()
    got, starts = windowed_loudness(xd, (W + 3) * step + 7, H * step, rate)
    nw = WR.num_windows(WR.num_complete_blocks(n, rate), W, H)
    assert got.shape == (rows, nw) and got.is_cuda and got.dtype == torch.float32 and starts == [w * H * step for w in range(nw)]
    again, _ = windowed_loudness(xd, (W + 3) * step, H * step, rate)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))  # deterministic; 7 samples more hold no further block
    _, blocks = integrated_loudness(xd, rate, return_blocks=True)
    got, blocks = got.double().cpu().numpy(), blocks.double().cpu().numpy()
    worst = 0.0
    for r in range(rows):
        want = ref[r][0]
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got[r]), fin) and np.all(np.isneginf(got[r][~fin]))
        worst = max(worst, float(np.max(np.abs(got[r][fin] - want[fin]))))
        for w, (_, a, f) in enumerate(ref[r][1]):
            assert WR.kernel_gate_sets(blocks[r], W, H, w) == (a, f), f"row {r} window {w}: gate sets differ"
    print(f"\n[{rows}x{chs}x{n} @ {rate}, W={W} H={H}] {nw} windows, |L - L_f64| = {worst:.3e} LU (bound {FP32_ALLOWANCE_LU:.1e})")
    assert worst <= FP32_ALLOWANCE_LU


def test_windows_against_the_meter_on_crops():
    """A window is the song's loudness there (warm filter); the meter on the crop starts its filter from rest.  How far apart the two
    may be is measured on the float64 restatement, window by window, on the same signal."""
    from mst.utils import integrated_loudness, windowed_loudness

    rate, step, rows = 44100, 4410, 3
    length, hop, n = 17640 + 10 * 4410, 5 * 4410, 17640 + 40 * 4410   # the crop has no partial block: 11 blocks, like the window
    x = (0.1 * np.random.default_rng(203).standard_normal((rows, 1, n)) * (10.0 ** (-0.7 * np.arange(rows) / 20.0))[:, None, None]).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    warm, starts = windowed_loudness(xd, length, hop, rate)
    assert starts == [w * hop for w in range(7)]
    crops = torch.as_strided(xd, (rows, len(starts), 1, length), (xd.stride(0), hop, xd.stride(1), 1))
    cold = integrated_loudness(crops, rate)
    assert cold.shape == warm.shape == (rows, 7)
    warm, cold = warm.double().cpu().numpy(), cold.double().cpu().numpy()
    for r in range(rows):
        ref_warm, _ = WR.windowed_loudness(x[r], rate, 11, 5)
        ref_cold = np.array([R.integrated_loudness(x[r, 0, s:s + length].astype(np.float64), rate) for s in starts])
        allowed = np.abs(ref_warm - ref_cold) + 2.0 * FP32_ALLOWANCE_LU
        diff = np.abs(warm[r] - cold[r])
        print(f"\n[row {r}] |window - meter on crop| = {np.array2string(diff, precision=2)} LU, restatement warm - cold "
              f"{np.array2string(np.abs(ref_warm - ref_cold), precision=2)}")
        assert np.all(diff <= allowed)
        assert abs(warm[r][0] - cold[r][0]) <= 2.0 * FP32_ALLOWANCE_LU  # window 0 starts from rest as well


@pytest.mark.parametrize("T,NW,count,gap", [(16, 5, 8, 1), (3, 257, 4, 30), (256, 4092, 64, 7)])
def test_picker_matches_the_numpy_rule(T, NW, count, gap):
    from mst import _hip

    track, mix, floor, mix_floor = S.random_tables(T, NW, 100 + T)
    want = S.pick_sections(track, mix, floor, mix_floor, count, gap)
    got = S.call_picker(_hip.lib(), torch.from_numpy(track).cuda(), torch.from_numpy(mix).cuda(), torch.from_numpy(floor).cuda(), mix_floor,
                        count, gap)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_a_synthetic_song_from_pick_to_fit():
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_sections, pick_sections, take_sections

    rate, n, length = 44100, 20 * 44100, 131072
    g = torch.Generator(device="cuda").manual_seed(204)
    noise = torch.randn(3, n, generator=g, device="cuda")
    tracks = torch.zeros(3, n, device="cuda")
    tracks[0] = 0.05 * noise[0]                                  # plays throughout
    tracks[1, 2 * rate:8 * rate] = 0.05 * noise[1, 2 * rate:8 * rate]
    tracks[2, 12 * rate:18 * rate] = 0.1 * noise[2, 12 * rate:18 * rate]
    pick = pick_sections(tracks, length, 2)
    print(f"\n[pick] starts {pick.starts}, mix {pick.mix_lufs.tolist()} LUFS")
    assert len(pick.starts) == 2 and pick.length == length and all(isinstance(s, int) for s in pick.starts)
    first, second = pick.starts
    blocks = (length // 4410) * 4410                             # the samples a window's complete gating blocks span
    assert 12 * rate <= first <= 18 * rate - blocks              # the louder interval first
    assert 2 * rate <= second <= 8 * rate - blocks
    assert pick.covered.tolist() == [True, True, True] and pick.active.tolist() == [[True, False, True], [True, True, False]]
    assert pick.track_lufs.shape == (3, 2) and pick.mix_lufs.shape == (2,) and pick.track_lufs.is_cuda
    assert torch.isneginf(pick.track_lufs[1, 0]) and torch.isneginf(pick.track_lufs[2, 1]) and pick.mix_lufs[0] > pick.mix_lufs[1] > -48.0
    # a floor no track reaches, and a mix floor no window reaches
    with pytest.raises(ValueError, match="eligible"):
        pick_sections(tracks, length, 2, track_floor_lufs=0.0)
    with pytest.raises(ValueError, match="eligible"):
        pick_sections(tracks, length, 2, mix_floor_lufs=0.0)
    alone = pick_sections(tracks, length, 4, track_floor_lufs=torch.tensor([0.0, -48.0, 0.0]), min_gap=3 * length)
    assert len(alone.starts) == 1 and alone.covered.tolist() == [False, True, False]  # one window of track 1; the next is too near

    sections = take_sections(tracks, pick.starts, pick.length)
    assert tuple(sections.shape) == (2, 3, length)
    ref = torch.stack((tracks[:, :length].sum(0), 0.5 * tracks[:, 12 * rate:12 * rate + length].sum(0)))
    seen = []
    torch.manual_seed(0)
    out = optimize_sections(sections, ref, AdvancedMixConsole(rate), AudioFeatureLoss([0.1, 0.001, 1.0, 1.0, 1.0], rate), n_iters=2,
                            callback=lambda i, view: seen.append(view.grads[0].clone()))
    assert len(seen) == 2 and tuple(out[0].shape) == (2, 2, length) and torch.isfinite(out[0]).all()
    for grad in seen:
        assert tuple(grad.shape) == (2, 3, 27) and torch.isfinite(grad).all()
        assert (grad.abs().sum(dim=(0, 2)) > 0).all()           # every track is heard in some section
