"""The logit-Adam kernels (diff-mst_amd/csrc/mst_opt.hip) on the host simulator, through the C ABI: (1) a whole gradient stream against
the float64 recurrence and torch.optim.Adam behind torch.sigmoid in fp32, (2) the sigmoid, (3) what must keep its bits, (4) non-finite
input, (5) the history rows.  Every buffer starts as NaN between guard regions (tests/online_ref.py).  tests/test_online_gpu.py carries
the same cases on the device."""
import ctypes

import pytest
import torch

import online_ref as R


@pytest.fixture()
def drv():
    from hostsim import harness

    return R.Driver(harness.lib(), "cpu")


@pytest.mark.parametrize("name", sorted(R.STREAMS))
def test_step_matches_adam_behind_sigmoid(drv, name, record):
    R.check_parity(drv, name, record)


@pytest.mark.parametrize("count", R.TAIL_COUNTS)
def test_lane_tails_and_the_loop(drv, count):
    R.check_parity(drv, str(count))


def test_sigmoid(drv, record):
    R.check_sigmoid(drv, record)


def test_null_gradient_and_zero_gradient_keep_their_bits(drv):
    R.check_unchanged_bits(drv)


@pytest.mark.parametrize("where", ["gradient", "loss"])
def test_nonfinite_input_stops_the_step_and_is_reported(drv, where):
    R.check_nonfinite(drv, where)


@pytest.mark.parametrize("n_terms", [1, 5])
def test_history_rows(drv, n_terms):
    R.check_history(drv, n_terms)


def test_unsupported_arguments_launch_nothing(drv):
    from mst import _cabi

    L = drv.lib
    assert L.mst_logit_adam_state_bytes(0) == 0 and L.mst_logit_adam_state_bytes((1 << 20) + 1) == 0
    assert L.mst_logit_adam_state_bytes(27 * 16 + 51) == 4 * (R.HDR + 2 * (27 * 16 + 51))
    theta, p, state, row, term = (drv.guarded(8) for _ in range(5))
    seg = (_cabi.LogitAdamSegment * 1)()
    seg[0].theta, seg[0].p, seg[0].grad_p, seg[0].count = theta.data_ptr(), p.data_ptr(), None, 8
    terms = (ctypes.c_void_p * 1)(term.data_ptr())
    good = dict(n_seg=1, terms=terms, n_terms=1, row=row, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, state=state)
    for change in (dict(n_seg=0), dict(n_seg=5), dict(n_terms=0), dict(n_terms=9), dict(terms=None), dict(row=None), dict(state=None),
                   dict(lr=0.0), dict(lr=float("nan")), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0)):
        a = dict(good, **change)
        with pytest.raises(_cabi.AbiError) as e:
            L.mst_logit_adam_step(seg, a["n_seg"], a["terms"], a["n_terms"], a["row"], a["lr"], a["b1"], a["b2"], a["eps"], a["state"], None)
        assert e.value.code != 0
    seg[0].count = 0
    with pytest.raises(_cabi.AbiError):
        L.mst_logit_adam_init(seg, 1, state, None)
    seg[0].count, seg[0].p = 8, None
    with pytest.raises(_cabi.AbiError):
        L.mst_logit_adam_init(seg, 1, state, None)
    for t in (theta, p, state, row, term):
        assert bool(torch.isnan(t).all())
    drv.check_guards()
