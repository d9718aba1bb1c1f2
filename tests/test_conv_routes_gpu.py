"""The encoder's convolution kernels one at a time on the device, per dispatch route: the case table of tests/conv_routes.py through the C
ABI's mst_conv3x3 / mst_conv_wgrad.  Integer operands make every kernel exact, so results are compared bit for bit with the float64
reference (torch.equal); the per-tile BatchNorm statistics and the low operand pieces of bf16x3 / bf16x6 hold bounds derived in
conv_routes' docstring.  Results, statistics, prepared weights, split-K slabs and partial weight gradients all start as NaN: no kernel
may rely on a cleared buffer and an element nobody writes fails the comparison."""
import ctypes

import pytest
import torch

import conv_routes as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mst import _hip

    _hip.lib()
    return torch.device("cuda:0")


def nan_bytes(dev, nbytes):
    """a device buffer of at least `nbytes` bytes, every 32-bit word a NaN (also as two bf16 values)"""
    return torch.full((max((nbytes + 3) // 4, 1),), float("nan"), device=dev)


def run_conv(dev, shape, precision, direction, ops, scratch=False, stats=False):
    """mst_conv3x3 on CPU operands -> (result on the host in its storage type, part on the host or None, tiles).  scratch: the split-K
    slabs the shape asks for are passed (a shape that is never split gets a small NaN buffer, which must come back untouched)."""
    from mst import _hip

    L = _hip.lib()
    n, h, w, cin, cout = shape
    dgrad = int(direction == "dgrad")
    st = torch.bfloat16 if precision == 0 else torch.float32
    src = ops["dy"] if dgrad else ops["x"]
    xd = (src if cin == 1 else src.to(st)).contiguous().to(dev)  # the first layer reads the fp32 spectrogram whatever the precision
    wd = ops["w"].contiguous().to(dev)
    kin, kout = (cout, cin) if dgrad else (cin, cout)
    out = torch.full((n, h, w, kout), float("nan"), dtype=st, device=dev)
    wsb = L.mst_conv3x3_workspace_bytes(precision, cin, cout)
    assert wsb > 0
    ws = nan_bytes(dev, wsb)
    need = L.mst_conv3x3_splitk_bytes(n, h, w, cin, cout, dgrad)
    assert need == (0 if cin == 1 else cr.splitk_bytes(n * h * w, kin, kout))
    sk = nan_bytes(dev, need or 4096) if scratch else None
    skb = (need or 4096) if scratch else 0
    pb = L.mst_conv3x3_part_bytes(n, h, w, cin, cout, dgrad)
    part = nan_bytes(dev, pb) if stats else None
    tiles = ctypes.c_int32(-1)
    with _hip.launch_on(dev) as stream:
        L.mst_conv3x3(precision, dgrad, xd, wd, out, part, ctypes.byref(tiles), n, h, w, cin, cout, ws, wsb, sk, skb, stream)
    torch.cuda.synchronize()
    if scratch and not need:
        assert bool(torch.isnan(sk).all()), "a convolution that is never split wrote to the split-K scratch"
    return out.cpu(), (part.cpu().view(-1, kout, 2) if stats else None), tiles.value


def run_wgrad(dev, shape, precision, ops):
    """mst_conv_wgrad on CPU operands -> (gradient (Cout, Cin, 3, 3) fp32 on the host, splits, steps per split, workspace bytes)"""
    from mst import _hip

    L = _hip.lib()
    n, h, w, cin, cout = shape
    st = torch.bfloat16 if precision == 0 else torch.float32
    dy = ops["dy"].to(st).contiguous().to(dev)
    x = (ops["x"] if cin == 1 else ops["x"].to(st)).contiguous().to(dev)
    gw = torch.full((cout, cin, 3, 3), float("nan"), device=dev)
    wsb = L.mst_conv_wgrad_workspace_bytes(precision, n, h, w, cin, cout)
    assert wsb > 0
    ws = nan_bytes(dev, wsb)
    splits, steps = ctypes.c_int32(-1), ctypes.c_int32(-1)
    with _hip.launch_on(dev) as stream:
        L.mst_conv_wgrad(precision, dy, x, gw, n, h, w, cin, cout, ws, wsb, ctypes.byref(splits), ctypes.byref(steps), stream)
    torch.cuda.synchronize()
    return gw.cpu(), splits.value, steps.value, wsb


def test_entries_refuse_what_the_kernels_are_not_written_for(dev):
    from mst import _cabi, _hip

    L = _hip.lib()
    assert L.mst_conv3x3_workspace_bytes(0, 64, 64) == 2 * 9 * 64 * 64 * 2 and L.mst_conv3x3_workspace_bytes(1, 1, 64) == 64 * 9 * 4
    assert L.mst_conv3x3_workspace_bytes(0, 96, 64) == 0 and L.mst_conv3x3_workspace_bytes(4, 64, 64) == 0 and L.mst_conv3x3_workspace_bytes(0, 1, 128) == 0
    assert L.mst_conv_wgrad_workspace_bytes(0, 1, 4, 4, 64, 4096) == 0
    t = torch.zeros(64 * 64 * 9, device=dev)
    for bad in (dict(cin=96), dict(precision=7), dict(n=0), dict(cin=1, dgrad=1)):
        a = dict(precision=1, dgrad=0, n=1, h=2, w=2, cin=64, cout=64)
        a.update(bad)
        with pytest.raises(_cabi.AbiError):
            L.mst_conv3x3(a["precision"], a["dgrad"], t, t, t, None, None, a["n"], a["h"], a["w"], a["cin"], a["cout"], t, t.numel() * 4, None, 0, None)
    with pytest.raises(_cabi.AbiError):  # workspace too small
        L.mst_conv3x3(1, 0, t, t, t, None, None, 1, 2, 2, 64, 64, t, 1024, None, 0, None)
    with pytest.raises(_cabi.AbiError):
        L.mst_conv_wgrad(1, t, t, t, 1, 2, 2, 64, 64, t, 1024, None, None, None)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in cr.CASES])
def test_conv_route_exact(case, dev):
    """One case of the table: the launcher takes the route the table states, as far as the ABI shows it (the tile count tells the 256-pixel
    kernels from the 128-pixel ones, the scratch size query the K split, the returned pixel split the weight-gradient plan), and the
    result equals the integer reference in every bit."""
    data = cr.reference(case.id)
    route = cr.route_by_rule(case)
    if case.direction == "wgrad":
        gw, splits, steps, wsb = run_wgrad(dev, case.shape, case.precision, data["ops"])
        assert (splits, steps) == case.split and wsb == 4 * cr.wgrad_floats(route, case.shape[3], case.shape[4])
        cr.grade_exact(case, gw, data["ref"])
        return
    out, _, tiles = run_conv(dev, case.shape, case.precision, case.direction, data["ops"], scratch=case.scratch)
    assert tiles == route.tiles
    cr.grade_exact(case, out, data["ref"])
    if case.direction == "fwd":
        cr.channel_sums(case.id)  # kept for the statistics test while the reference is at hand


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in cr.STATS_CASES])
def test_conv_route_statistics(case, dev, record):
    """The per-tile sum and sum of squares BatchNorm folds: every tile of the route's tile size written, the float64 fold within
    256 x 2^-24 x sum |v| (sum v^2) of the exact sums, per channel - on the unsplit kernels, the 256-pixel kernels, k_conv1, and the
    split-K reduce, which forms the statistics itself."""
    sums = cr.channel_sums(case.id)
    out, part, tiles = run_conv(dev, case.shape, case.precision, case.direction, cr.draw(case), scratch=case.scratch, stats=True)
    assert tiles == cr.route_by_rule(case).tiles
    used = cr.grade_stats(case, part, tiles, sums)
    assert bool(torch.isnan(part[tiles:]).all())  # nothing written past the tiles the launcher reports
    assert not torch.isnan(out.float()).any()
    record(sum_over_bound=used[0], sumsq_over_bound=used[1])


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in cr.PIECE_CASES])
def test_low_pieces(case, dev, record):
    """One product per result, full-mantissa operands: the kernel's value is the fp32 sum of exactly the terms mma_split keeps - a dropped
    or mispaired cross term is 2^-9 (x3) or 2^-17 (x6) of the product, far outside TERMS x 2^-24.  The distance to the true product is
    recorded, not graded (profiles/conv_routes.md)."""
    ops = cr.draw_pieces(case)
    if case.direction == "wgrad":
        out = run_wgrad(dev, case.shape, case.precision, ops)[0]
    else:
        out = run_conv(dev, case.shape, case.precision, case.direction, ops)[0]
    of_bound, per_product = cr.grade_pieces(case, out, ops)
    print(f"\n[conv pieces {case.id}] max |out - kept| / bound {of_bound:.3f}; max |out - a b| / |a b| {per_product:.3e} = 2^{torch.tensor(per_product).log2().item():.2f}")
    record(of_bound=of_bound, per_product=per_product)
