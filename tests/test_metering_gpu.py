"""The delivery meter on the MI355X through its Python surface (mst.utils: true_peak, short_term_loudness, loudness_range,
meter_report, loudness_normalize_limited) against the float64 restatement (tests/metering_ref.py; parity with any external meter is
UNPINNED).  Bounds and the gate-margin pre-check are those of tests/test_metering_hostsim.py."""
import math

import numpy as np
import pytest
import torch

import loudness_ref as R
import metering_ref as M

pytestmark = pytest.mark.gpu

FP32_ALLOWANCE_LU = 8.7e-5   # derived in tests/test_loudness_hostsim.py
GATE_MARGIN_LU = 1e-3
RATE = 44100
DB_PER_REL = 20.0 / math.log(10.0)  # a relative error e of a linear value is e * 8.69 dB


def taps(F):
    from mst import _hip

    return M.lib_taps(_hip.lib(), F)


def check_true_peak_db(got_db, x, rate, label):
    """got_db (rows, channels) dBTP from the device; x numpy (rows, channels, n).  The linear bound of the simulator tests, in dB."""
    F = M.factor_of(rate)
    h = taps(F)
    worst = 0.0
    for r in range(x.shape[0]):
        for c in range(x.shape[1]):
            ref = M.true_peak(x[r, c:c + 1], h, F)
            bound = M.true_peak_bound(h, F, float(np.max(np.abs(x[r, c]))))
            # 20 log10 in fp32 on the device: one rounding of a value of at most a few tens of dB, 2^-23 * 64 covers it
            tol = DB_PER_REL * bound / ref + 64.0 * 2.0 ** -23
            err = abs(float(got_db[r, c]) - float(M.dbtp(ref)))
            worst = max(worst, err / tol)
            assert err <= tol, f"{label} item {r} channel {c}: {err:.3e} dB > {tol:.3e} dB"
    print(f"\n[{label}] worst error / bound = {worst:.3f}")


@pytest.fixture(scope="module")
def small():
    from mst._cabi import TRUE_PEAK_TILE as TILE

    n = 3 * TILE + 5
    rng = np.random.default_rng(11)
    return (0.3 * rng.standard_normal((3, 2, n)) * (10.0 ** (-0.35 * np.arange(3)))[:, None, None]).astype(np.float32)


@pytest.fixture(scope="module")
def production():
    """(2, 2, 524288) level-step noise and its restatement, computed once: true peaks per channel, short-term energies at H = 10."""
    x = R.level_step_noise(2, 2, 524288, 301)
    h = taps(4)
    tp = np.array([[M.true_peak(x[r, c:c + 1], h, 4) for c in range(2)] for r in range(2)])
    st = [M.short_term(x[r], RATE, 10) for r in range(2)]
    return x, tp, st


def test_true_peak_small_shape_and_both_factors(small):
    from mst.utils import true_peak

    dev = torch.device("cuda:0")
    x = torch.from_numpy(small).to(dev)
    for rate in (44100, 96000):
        per = true_peak(x, rate, per_channel=True)
        item = true_peak(x, rate)
        assert per.shape == (3, 2) and item.shape == (3,) and per.is_cuda and torch.equal(item, per.amax(dim=1))
        assert torch.equal(per, true_peak(x, rate, per_channel=True))  # deterministic
        check_true_peak_db(per.double().cpu().numpy(), small, rate, f"3x2x{small.shape[2]} @ {rate}")


def test_production_shape_matches_the_restatement(production):
    from mst.utils import loudness_range, short_term_loudness, true_peak

    dev = torch.device("cuda:0")
    x, tp, st = production
    xd = torch.from_numpy(x).to(dev)
    per = true_peak(xd, RATE, per_channel=True).double().cpu().numpy()
    check_true_peak_db(per, x, RATE, "2x2x524288 true peak")
    assert np.max(np.abs(per - M.dbtp(tp))) < 1e-4
    short, starts = short_term_loudness(xd)
    lra, bounds = loudness_range(xd, return_bounds=True)
    assert short.shape == (2, len(starts)) and starts == [k * RATE for k in range((524288 // 4410 - 30) // 10 + 1)]
    short, lra, bounds = short.double().cpu().numpy(), lra.double().cpu().numpy(), bounds.double().cpu().numpy()
    lost_abs = lost_rel = False
    for r in range(2):
        E, l = st[r]
        want, l_lo, l_hi, a, f = M.loudness_range(E)
        m_rel, m_abs = M.range_margins(l)
        assert m_rel > GATE_MARGIN_LU and m_abs > GATE_MARGIN_LU, f"row {r}: a window sits on a gate, change the seed"
        lost_abs |= len(a) < len(E)
        lost_rel |= len(f) < len(a)
        above = l > -70.0
        err = float(np.max(np.abs(short[r] - l)[above]))
        ga, _, gf = M.range_gates(short[r])
        assert (ga, gf) == (a, f)
        err_r = max(abs(lra[r] - want), abs(bounds[r, 0] - l_lo), abs(bounds[r, 1] - l_hi))
        print(f"\n[2x2x524288 row {r}] |l_k - l_k_f64| = {err:.3e} LU, |LRA - LRA_f64| = {err_r:.3e} LU (bound {FP32_ALLOWANCE_LU:.1e})")
        assert err <= FP32_ALLOWANCE_LU and err_r <= FP32_ALLOWANCE_LU
    assert lost_abs and lost_rel


def test_meter_report_agrees_with_the_single_functions(production):
    from mst.utils import (LoudnessReport, integrated_loudness, loudness_range, meter_report, momentary_loudness, short_term_loudness,
                           true_peak)

    xd = torch.from_numpy(production[0]).to("cuda:0")
    rep = meter_report(xd)
    assert isinstance(rep, LoudnessReport) and all(t.shape == (2,) and t.is_cuda for t in rep)
    assert torch.equal(rep.integrated, integrated_loudness(xd))
    assert torch.equal(rep.loudness_range, loudness_range(xd))
    assert torch.equal(rep.momentary_max, momentary_loudness(xd).amax(dim=-1))
    assert torch.equal(rep.short_term_max, short_term_loudness(xd)[0].amax(dim=-1))
    assert torch.equal(rep.true_peak, true_peak(xd))
    assert torch.equal(rep.sample_peak, 20.0 * torch.log10(xd.abs().amax(dim=(1, 2))))
    assert (rep.true_peak >= rep.sample_peak).all() and (rep.short_term_max <= rep.momentary_max + 1e-3).all()


def test_leading_dimensions_and_strided_crops_are_read_in_place(small):
    from mst.utils import loudness_range, short_term_loudness, true_peak

    dev = torch.device("cuda:0")
    n = small.shape[2]
    long = torch.zeros(3, 2, n + 9, device=dev)
    long[..., 3:3 + n] = torch.from_numpy(small).to(dev)
    crop = long[..., 3:3 + n]                    # rows at odd element offsets
    assert not crop.is_contiguous()
    a = true_peak(crop, per_channel=True)
    assert torch.equal(a, true_peak(torch.from_numpy(small).to(dev), per_channel=True))
    six = torch.from_numpy(small).to(dev).view(3, 2, 1, n)      # leading dimensions (3, 2), one channel
    assert torch.equal(true_peak(six), a)
    assert true_peak(crop[0]).shape == () and torch.equal(true_peak(crop[0]), a[0].amax())
    x = torch.from_numpy(R.level_step_noise(4, 1, 31 * 4410 + 7, 302)).to(dev)
    wide = torch.zeros(4, 1, x.shape[2] + 6, device=dev)
    wide[..., 5:5 + x.shape[2]] = x
    view = wide[..., 5:5 + x.shape[2]]
    s, starts = short_term_loudness(view, hop=4410)
    assert s.shape == (4, 2) and starts == [0, 4410] and torch.equal(s, short_term_loudness(x, hop=4410)[0])
    r = loudness_range(view.view(2, 2, 1, -1) if view.is_contiguous() else view.reshape(2, 2, 1, -1), hop=4410)
    assert r.shape == (2, 2) and torch.equal(r.flatten(), loudness_range(x, hop=4410))
    with pytest.raises(NotImplementedError):
        true_peak(crop.clone().requires_grad_())


def test_a_non_default_stream(small):
    from mst.utils import loudness_range, true_peak

    dev = torch.device("cuda:0")
    x = torch.from_numpy(small).to(dev)
    y = torch.from_numpy(R.level_step_noise(2, 2, 31 * 4410, 303)).to(dev)
    tp, lra = true_peak(x, per_channel=True), loudness_range(y)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        tp_s, lra_s = true_peak(x, per_channel=True), loudness_range(y)
    side.synchronize()
    assert torch.equal(tp_s, tp) and torch.equal(lra_s, lra)


def test_loudness_normalize_limited_end_to_end():
    from mst.utils import integrated_loudness, loudness_normalize, loudness_normalize_limited, true_peak

    dev = torch.device("cuda:0")
    n, target, ceiling = 70001, -14.0, -1.0
    g = torch.Generator().manual_seed(5)
    x = torch.zeros(4, 2, n)
    x[0] = 0.003 * torch.randn(2, n, generator=g)
    x[0, 1, 30000:30002] = 0.6                       # sparse: the loudness gain would push its peak far over full scale
    x[1] = 0.02 * torch.randn(2, n, generator=g)     # dense and quiet enough to reach -14 LUFS below the ceiling
    x[3] = 1e-5 * torch.randn(2, n, generator=g)     # below the floor
    x = x.to(dev)
    y, lufs, keep, gain, tp = loudness_normalize_limited(x, target, ceiling, floor_lufs=-80.0)
    plain, plufs, pkeep = loudness_normalize(x, target, floor_lufs=-80.0)
    assert y.shape == x.shape and keep.tolist() == pkeep.tolist() == [True, True, False, False]
    assert torch.equal(lufs, plufs) and torch.equal(tp, true_peak(x))
    assert not y[2].any() and not y[3].any() and torch.isneginf(gain[2:]).all()
    l64, tp64, g64 = lufs.double().cpu(), tp.double().cpu(), gain.double().cpu()
    assert target - l64[0] > ceiling - tp64[0] and target - l64[1] < ceiling - tp64[1]
    # tp is 20 log10 in fp32 of the linear value the kernel used: its rounding (2^-23 of a few dB) is all that separates the two
    assert abs(g64[0] - (ceiling - tp64[0])) <= 1e-5 and abs(g64[1] - (target - l64[1])) <= 2.0 ** -22 * abs(g64[1])
    assert torch.equal(y[1], plain[1])
    after = true_peak(y[:2]).double().cpu()
    h = taps(4)
    lin = 10.0 ** (ceiling / 20.0)
    for r in (0, 1):  # the slack derived in tests/test_metering_hostsim.py::test_normalize_limited, in dB
        ymax = float(y[r].abs().max())
        slack = lin * 2.0 ** -22 + 2.0 ** -24 * M.sum_abs_taps(h, 4) * ymax + M.true_peak_bound(h, 4, ymax)
        print(f"\n[limited item {r}] gain {float(g64[r]):+.4f} dB, true peak after {float(after[r]):+.5f} dBTP (ceiling {ceiling})")
        assert float(after[r]) <= ceiling + DB_PER_REL * slack / lin + 64.0 * 2.0 ** -23
    assert abs(float(after[0]) - ceiling) < 1e-4
    assert abs(float(integrated_loudness(y[1])) - target) < 1e-4
