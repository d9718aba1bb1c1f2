"""The MR-STFT route table (tests/mrstft_routes.py) on the host simulator: the unchanged kernel sources of mst_stft.hip / mst_stft2.hip
through the C ABI, graded like the device tests.  The cases that take the simulator 40 s or more are `slow` here (one of them, 258 rows,
is left to the device altogether); all of them run on the GPU in tests/test_mrstft_routes_gpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "hostsim"))
import harness  # noqa: E402
import mrstft_routes as mr  # noqa: E402

SIM_CASES = [pytest.param(c, id=c.id, marks=[pytest.mark.slow] if c.sim == "slow" else []) for c in mr.CASES if c.sim != "never"]


def test_the_table_follows_the_dispatch_rules():
    """Every case's stated route is the one the rules of the module docstring give for its shape, and the table reaches every route."""
    for c in mr.CASES:
        assert (c.fast_flags, c.bwd) == mr.route_by_rule(c), c.id
        assert len(c.why) > 10
    assert {c.bwd for c in mr.CASES} == {"generic", "own", "own+fused", "zero", "seam", "seam+fused"}
    assert {r[0] for c in mr.CASES for r, f in zip(c.res, c.fast_flags) if not f} == {128, 256, 512, 1024, 2048, 4096, 8192}
    assert mr.unreached(mr.BY_ID["g512_hop700_n5000"])[:4500].sum() > 1000  # gaps between frames, not only the dropped tail of the row


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in mr.CASES])
def test_plan_takes_the_stated_route(case):
    """What the C ABI shows of a plan is its workspace size: a resolution on the fast kernels keeps two planes, a seam hand-over has its
    slab.  (Whether 512 + 2048 share one backward launch, and how the strips are laid out, cannot be observed through the ABI.)"""
    from mst.loss import _mrstft_desc

    d = _mrstft_desc(case.n_rows, case.n, case.res, 1.0, 0.0, 0.0, True, 1e-8)
    assert harness.lib().mst_mrstft_workspace_bytes(d) == 4 * mr.workspace_floats(case)


@pytest.mark.parametrize("case", SIM_CASES)
def test_mrstft_route(case):
    ref = mr.reference(case.id)
    out = harness.mrstft(ref["x"], ref["y"], case.res, **case.kw)
    mr.grade(case, out["loss"].item(), out["grad_pred"])


@pytest.mark.parametrize("res,n", [(mr.R3, 16384), (mr.R3, 4097)], ids=["fast", "generic"])
def test_zero_prediction(res, n):
    """An all-zero prediction: every bin of it sits below the 1e-8 clamp, so the loss (log term included) is finite and the gradient is
    exactly zero, on both engines."""
    torch.manual_seed(n)
    y = 0.3 * torch.randn(1, 2, n)
    x = torch.zeros_like(y)
    out = harness.mrstft(x, y, res)
    l64, _ = mr.oracle(x, y, res, {}, torch.float64)
    assert abs(out["loss"].item() - l64) / l64 < 1e-5
    assert torch.equal(out["grad_pred"], torch.zeros_like(x))
