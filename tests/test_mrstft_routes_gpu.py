"""The MR-STFT loss on the device at every transform size and on every dispatch route: the case table of tests/mrstft_routes.py through
the C ABI (gradient buffer, tables and workspace start as NaN), and the Python class for what only it does (the upstream gradient, the
prediction's dtype and layout).  Shapes are small on purpose - at most 33 000 samples by 6 rows, one case of 258 rows: one wrong sample
then moves every graded figure by 1e-3 or more, and nearly all of a case's time is the host oracle."""
import pytest
import torch

import mrstft_routes as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mst import _hip

    _hip.lib()
    return torch.device("cuda:0")


def hip_call(dev, x, y, res, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, sc_per_example=True):
    """tests/hostsim/harness.py::mrstft on the device: (bs, chs, n) CPU tensors -> (loss, gradient on the host, workspace bytes).  Every
    buffer the library writes starts as NaN: an element no kernel writes, or a workspace word read before it is written, shows."""
    from mst import _hip
    from mst.loss import _mrstft_desc

    L = _hip.lib()
    n = x.shape[-1]
    xd = x.reshape(-1, n).contiguous().float().to(dev)
    yd = y.reshape(-1, n).contiguous().float().to(dev)
    d = _mrstft_desc(xd.shape[0], n, res, w_sc, w_log_mag, w_lin_mag, sc_per_example, 1e-8)
    tb, wb = L.mst_mrstft_tables_bytes(d), L.mst_mrstft_workspace_bytes(d)
    assert tb > 0 and wb > 0

    def nan(count):
        return torch.full((count,), float("nan"), device=dev)

    tables, ws, loss, gx = nan(tb // 4), nan(wb // 4), nan(1), torch.full_like(xd, float("nan"))
    gl = torch.ones(1, device=dev)
    with _hip.launch_on(dev) as st:
        L.mst_mrstft_init_tables(d, tables, st)
        L.mst_mrstft_forward(d, xd, yd, tables, loss, ws, wb, st)
        L.mst_mrstft_backward(d, xd, yd, tables, gl, gx, ws, wb, st)
    return loss.item(), gx.cpu().view_as(x), wb


def make_loss(res, **kw):
    from mst.loss import MultiResolutionSTFTLoss

    return MultiResolutionSTFTLoss(fft_sizes=[r[0] for r in res], hop_sizes=[r[1] for r in res], win_lengths=[r[2] for r in res], **kw)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in mr.CASES])
def test_mrstft_route(case, dev, record):
    """One case of the table: the plan takes the route the table states - as far as the C ABI shows it, which is the workspace size (two
    kept planes per resolution on the fast kernels, the slab of a seam hand-over; whether 512 + 2048 share a backward launch and how the
    strips are cut is not observable through the ABI and follows from the case's shape by the rules in mrstft_routes) - and loss and
    gradient hold the table's bounds.  A second call must give the same loss bits on every route and the same gradient bits wherever
    the backward runs on the fast kernels (owner-computes, or exactly two atomic contributions per sample onto zeros); the generic
    backward overlap-adds with float atomics in no fixed order and is exempt."""
    ref = mr.reference(case.id)
    loss, grad, wb = hip_call(dev, ref["x"], ref["y"], case.res, **case.kw)
    assert wb == 4 * mr.workspace_floats(case)
    mr.grade(case, loss, grad, record)
    loss2, grad2, _ = hip_call(dev, ref["x"], ref["y"], case.res, **case.kw)
    assert loss2 == loss
    if case.bwd != "generic":
        assert torch.equal(grad2, grad)
    else:
        assert torch.isfinite(grad2).all()


@pytest.mark.parametrize("case_id", ["r3_rows1x1_n16384", "r3_n4097"], ids=["fast", "generic"])
def test_upstream_gradient_scales_the_result(case_id, dev, record):
    """(3 loss).backward() through the Python class: the kernels fold dL/dloss into their coefficients; same bounds, against 3 x the
    oracle's gradient."""
    case, ref = mr.BY_ID[case_id], mr.reference(case_id)
    xd = ref["x"].to(dev).requires_grad_(True)
    loss = make_loss(case.res, **case.kw)(xd, ref["y"].to(dev))
    (3.0 * loss).backward()
    mr.grade(case, loss.item(), xd.grad, record, scale=3.0, what=" x 3")


@pytest.mark.parametrize("how", ["float16", "bfloat16", "float64", "strided"])
def test_prediction_dtype_and_layout(how, dev):
    """A half, bfloat16, double or non-contiguous (strided crop) prediction is the same call as its values in contiguous fp32: the
    bit-identical loss, and the fp32 call's gradient cast to the prediction's dtype, in its shape.  On the all-fast route, whose
    backward has no atomics left, so that 'the same' can mean bit for bit."""
    n = 16384
    torch.manual_seed(77)
    wide = (0.3 * torch.randn(1, 2, n + 96)).to(dev)
    y = (0.5 * wide[..., 40:40 + n] + 0.2 * torch.randn(1, 2, n, device=dev)).contiguous()
    if how == "strided":
        x = wide[..., 40:40 + n].detach()
        assert not x.is_contiguous()
    else:
        x = wide[..., 40:40 + n].contiguous().to(getattr(torch, how))
    x.requires_grad_(True)
    plain = x.detach().float().contiguous().requires_grad_(True)
    f = make_loss(mr.R3)
    l_plain = f(plain, y)
    l_plain.backward()
    loss = f(x, y)
    loss.backward()
    assert loss.dtype == torch.float32 and torch.equal(loss.detach(), l_plain.detach())
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    assert torch.isfinite(plain.grad).all() and float(plain.grad.abs().max()) > 0
    assert torch.equal(x.grad, plain.grad.to(x.dtype))


@pytest.mark.parametrize("res,n", [(mr.R3, 16384), (mr.R3, 4097)], ids=["fast", "generic"])
def test_zero_prediction(res, n, dev):
    """An all-zero prediction against a non-zero target: every bin of it sits below the 1e-8 clamp, so the loss (log term included) is
    finite and the gradient exactly zero, on both engines."""
    torch.manual_seed(n)
    y = 0.3 * torch.randn(1, 2, n)
    x = torch.zeros_like(y)
    l64, _ = mr.oracle(x, y, res, {}, torch.float64)
    loss, grad, _ = hip_call(dev, x, y, res)
    assert abs(loss - l64) / l64 < 1e-5
    assert torch.equal(grad, torch.zeros_like(x))
    xd = x.to(dev).requires_grad_(True)
    via_class = make_loss(res)(xd, y.to(dev))
    via_class.backward()
    assert via_class.item() == loss and torch.equal(xd.grad.cpu(), torch.zeros_like(x))
