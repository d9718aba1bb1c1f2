"""The per-item MR-STFT loss (mst_mrstft_forward_items / _backward_items, include/diffmst_hip.h): the calls through a bound library, the
input recipe and the per-item oracles shared by tests/test_mrstft_items_hostsim.py (the host simulator: `sim()`) and
tests/test_mrstft_items_gpu.py (the device: `dev()`).  A plain module, no conftest.

Rows are item-major: a `(items, R)` shape means `items * R` rows of which item b owns rows b R .. b R + R - 1.  Inputs follow the recipe
of mrstft_routes.draw (x = 0.3 randn, y = 0.5 x + 0.2 randn, a seed per case id); every item is graded by mrstft_routes.grade against
oracle.loss_restated.mrstft_loss evaluated on that item's rows alone, in float64 and in float32: loss < 1e-5, gradient h <= 2 r + 1e-5
in rel-L2 and per sample.  Gradient buffers and workspaces start as NaN."""
import functools
import os
import sys
import zlib
from types import SimpleNamespace

import torch

import mrstft_routes as mr

R5 = ((128, 32, 128), (128, 64, 100), (256, 64, 256), (256, 128, 255), (256, 32, 200))  # five small resolutions (all generic)
STAGED = 640  # (resolution, row) entries the item reduction stages in LDS (kItemStage, mst_stft.h)


def sim():
    """the host simulator's library"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))
    import harness

    return SimpleNamespace(lib=harness.lib(), device=torch.device("cpu"), stream=lambda: _Null())


def dev():
    """the product library on cuda:0"""
    from mst import _hip

    d = torch.device("cuda:0")
    return SimpleNamespace(lib=_hip.lib(), device=d, stream=lambda: _hip.launch_on(d))


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


LIN_TAU = 2e-6


def lin_mag_well_posed(x, y, res):
    """Whether the linear-magnitude term's gradient is defined to fp32 accuracy on this draw, judged on the float64 spectra alone.  Its
    cotangent is sign(|X| - |Y|) per bin: a bin where the two magnitudes agree to within the round-off of an fp32 transform has a
    sign that ANY fp32 evaluation may take either way, and one flipped bin moves the gradient of rows this short by 1e-3 (the scalar
    loss on such a row alone shows it: measured 2.6e-3 against 3e-7 on the bin-free rows of the same draw).  An fp32 radix transform
    of N points carries about eps log2 N = 6e-8 x 13 = 8e-7 of the row's rms bin magnitude, the difference of two magnitudes twice
    that: a draw is well posed when no bin has ||X| - |Y|| < LIN_TAU = 2e-6 x that rms."""
    from oracle import loss_restated as ol

    for n_fft, hop, win in res:
        xm, ym = ol.stft_mag(x.double(), n_fft, hop, win), ol.stft_mag(y.double(), n_fft, hop, win)
        rms = (ym ** 2).mean(dim=(-1, -2), keepdim=True).sqrt()
        if bool(((xm - ym).abs() < LIN_TAU * rms).any()):
            return False
    return True


@functools.lru_cache(maxsize=None)
def draw(case_id, items, per_item, n, lin_res=None):
    """mrstft_routes.draw's recipe with a seed per case id; shared, never modified.  `lin_res` (the resolutions, for a case with the
    linear-magnitude term): the first of the seeds crc, crc + 1, ... whose draw is `lin_mag_well_posed`."""
    seed = zlib.crc32(case_id.encode()) & 0xFFFF
    for k in range(64):
        torch.manual_seed(seed + k)
        x = 0.3 * torch.randn(items * per_item, n)
        y = 0.5 * x + 0.2 * torch.randn(items * per_item, n)
        if lin_res is None or lin_mag_well_posed(x, y, lin_res):
            return x, y
    raise AssertionError(f"{case_id}: no well-posed draw in 64 seeds")


class Call:
    """One descriptor's tables and a NaN workspace on a backend; `forward_items` / `backward_items` / `forward` / `backward` are the
    C ABI's calls on (rows, n) host tensors, results back on the host."""

    def __init__(self, be, x, y, res, kw):
        from mst.loss import _mrstft_desc

        self.be, self.L = be, be.lib
        k = dict(w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, sc_per_example=True)
        k.update(kw)
        self.rows, self.n = x.shape
        self.d = _mrstft_desc(self.rows, self.n, res, k["w_sc"], k["w_log_mag"], k["w_lin_mag"], k["sc_per_example"], 1e-8)
        self.tb, self.wb = self.L.mst_mrstft_tables_bytes(self.d), self.L.mst_mrstft_workspace_bytes(self.d)
        assert self.tb > 0 and self.wb > 0
        self.x, self.y = x.contiguous().float().to(be.device), y.contiguous().float().to(be.device)
        self.tables = torch.full((self.tb // 4,), float("nan"), device=be.device)
        with be.stream() as st:
            self.L.mst_mrstft_init_tables(self.d, self.tables, st)
        self.fresh()

    def fresh(self):
        ws = torch.full((self.wb // 4 + 64,), float("nan"), device=self.be.device)
        self.ws = ws[(-ws.data_ptr() % 256) // 4:]

    def _nan(self, *shape):
        return torch.full(shape, float("nan"), device=self.be.device)

    def forward_items(self, items, keep=True):
        out = self._nan(max(items, 1))
        fn =self.L.mst_mrstft_forward_items if keep else self.L.mst_mrstft_forward_items_eval
        with self.be.stream() as st:
            fn(self.d, items, self.x, self.y, self.tables, out, self.ws, self.wb, st)
        return out.cpu()

    def backward_items(self, items, g):
        gx = self._nan(self.rows, self.n)
        g = torch.as_tensor(g, dtype=torch.float32).reshape(-1).to(self.be.device)
        with self.be.stream() as st:
            self.L.mst_mrstft_backward_items(self.d, items, self.x, self.y, self.tables, g, gx, self.ws, self.wb, st)
        return gx.cpu()

    def forward(self):
        out = self._nan(1)
        with self.be.stream() as st:
            self.L.mst_mrstft_forward(self.d, self.x, self.y, self.tables, out, self.ws, self.wb, st)
        return out.cpu()

    def backward(self, g):
        gx = self._nan(self.rows, self.n)
        g = torch.tensor([g], dtype=torch.float32).to(self.be.device)
        with self.be.stream() as st:
            self.L.mst_mrstft_backward(self.d, self.x, self.y, self.tables, g, gx, self.ws, self.wb, st)
        return gx.cpu()


def items_call(be, x, y, res, kw, items, g=None):
    """forward_items + backward_items (unit cotangents unless `g`) -> (losses (items,), gradient (rows, n))"""
    c = Call(be, x, y, res, kw)
    losses = c.forward_items(items)
    return losses, c.backward_items(items, torch.ones(items) if g is None else g)


@functools.lru_cache(maxsize=None)
def item_reference(case_id, items, per_item, n, res, kw_items, b):
    """Inputs and both oracles of item b of a drawn case, in the form mrstft_routes.grade takes: computed once per session, shared."""
    kw = dict(kw_items)
    x, y = draw(case_id, items, per_item, n, res if kw.get("w_lin_mag") else None)
    xb, yb = x[b * per_item:(b + 1) * per_item], y[b * per_item:(b + 1) * per_item]
    l64, g64 = mr.oracle(xb, yb, res, kw, torch.float64)
    l32, g32 = mr.oracle(xb, yb, res, kw, torch.float32)
    return dict(x=xb, y=yb, l64=l64, g64=g64, l32=l32, g32=g32)


def grade_items(case_id, items, per_item, n, res, kw, losses, grad, which=None):
    """Every item (or the items `which`) of a call's result against its own oracle, by mrstft_routes.grade."""
    for b in (range(items) if which is None else which):
        ref = item_reference(case_id, items, per_item, n, res, tuple(sorted(kw.items())), b)
        case = mr.Case(f"{case_id}[{b}]", res, n, "item %d of %d on its own rows" % (b, items), rows=(1, per_item), fast="?", bwd="?", kw=kw)
        mr.grade(case, losses[b].item(), grad[b * per_item:(b + 1) * per_item], ref=ref, what=f" item {b}/{items} R {per_item}")


# ---- the checks, shared by the simulator and the device test files -----------------------------------------------------------------
ONE_ITEM_ROUTES = ("r3_rows3x1_n20480", "r2_n4096", "g256_win255_n777", "r3_8192_first_n21504", "g512_g1024_global_sc_rows3x2_n3000",
                   "g512_g256_lin_mag_n3000")
SHAPES = ((2, 2), (3, 1), (2, 6), (5, 2))  # (items, R)
GENERIC2 = ((512, 128, 400), (1024, 256, 1024))
LENGTHS = {"n16384_fast": (16384, mr.R3), "n4352_mixed": (4352, mr.R3), "n3000_generic": (3000, GENERIC2)}
KWS = {"per_example": dict(mr.SMOOTH), "global_sc": dict(mr.GLOBAL_SC), "lin_mag": dict(w_sc=1.0, w_log_mag=0.0, w_lin_mag=1.0)}


def ordered(res, n):
    """Whether the backward of this shape writes every gradient sample in a fixed order: true on the owner-computes routes (every
    resolution on the register-radix kernels), false on the generic route, whose overlap-add is float atomics in the order the
    hardware - or the simulator's threads - happens to issue them: there mst_mrstft_backward does not reproduce its own bits from
    one call to the next, so no call can be compared with it bit for bit."""
    return mr.route_by_rule(mr.Case("route", res, n, ""))[1] != "generic"


def slabs(call, res, n):
    """The workspace's row sums, the two coefficient slabs (n_res, rows, 4) and the ticket region's 64 words, as the plan lays them
    out (mrstft_routes.workspace_floats: partial sums | row sums | coefficients | scaled coefficients | tickets)."""
    fast, rows = mr.route_by_rule(mr.Case("route", res, n, ""))[0], call.rows
    part = 0
    for (nf, hop, _), f in zip(res, fast):
        frames = 1 + n // hop
        groups = max(frames // {512: 3, 2048: 6, 8192: 5}[nf], 1) if f else ((frames + 1) // 2 if frames * rows >= 1024 else frames)
        part += rows * groups * 4
    at, size = (part + 63) // 64 * 64, len(res) * rows * 4
    step = (size + 63) // 64 * 64
    ws = call.ws.cpu()
    return SimpleNamespace(sums=ws[at:at + size].clone(), coef=ws[at + step:at + step + size].clone(),
                           scaled=ws[at + 2 * step:at + 2 * step + size].clone(), tickets=ws[at + 3 * step:at + 3 * step + 64].clone())


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_one_item_is_the_scalar_loss(be, case_id, g=0.7):
    """items = 1 under a cotangent that is no power of two.  The loss, the row sums and the backward coefficients have the bits of
    mst_mrstft_forward's; what the backward launches multiply - the scaled slab times a device 1.0f - has the bits of the products
    mst_mrstft_backward's launches form (coefficient x cotangent, one fp32 product); and where the backward's writes are ordered
    (`ordered`) the gradient has mst_mrstft_backward's bits.  On the generic route two calls of mst_mrstft_backward itself differ in
    the last bits (measured on the simulator: up to 1.4e-7 of the peak, all four generic cases, every repeat; the device tests of
    tests/test_mrstft_routes_gpu.py exempt that route from their second-call comparison for the same reason), so there the gradient
    is held to the suite's bounds against g x the float64 oracle instead."""
    case = mr.BY_ID[case_id]
    ref = mr.reference(case_id)
    x, y = ref["x"].reshape(-1, case.n), ref["y"].reshape(-1, case.n)
    c = Call(be, x, y, case.res, case.kw)
    loss, grad = c.forward(), c.backward(g)
    scalar = slabs(c, case.res, case.n)
    c.fresh()
    loss_items, grad_items = c.forward_items(1), c.backward_items(1, [g])
    items = slabs(c, case.res, case.n)
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    assert torch.equal(loss_items, loss), (loss_items, loss)
    assert same_bits(items.sums, scalar.sums) and same_bits(items.coef, scalar.coef)
    coef3 = scalar.coef.view(-1, 4)[:, :3]
    assert torch.isfinite(coef3).all()
    assert same_bits(items.scaled.view(-1, 4)[:, :3] * items.tickets[1], coef3 * torch.tensor(g, dtype=torch.float32))
    assert items.tickets[1].item() == 1.0
    if ordered(case.res, case.n):
        assert torch.equal(grad_items, grad), float((grad_items - grad).abs().max())
    else:
        mr.grade(case, loss_items.item(), grad_items, scale=g, what=f" items=1, cotangent {g}")


def check_every_item(be, shape, length, kw_name):
    items, per_item = shape
    n, res = LENGTHS[length]
    kw = KWS[kw_name]
    case_id = f"items{items}x{per_item}_{length}"
    x, y = draw(case_id, items, per_item, n, res if kw.get("w_lin_mag") else None)
    losses, grad = items_call(be, x, y, res, kw, items)
    grade_items(case_id, items, per_item, n, res, kw, losses, grad)


def check_isolation(be, length):
    """three stereo items; item 1 replaced, then poisoned, then given a zero cotangent: the others keep the bits of their losses
    and - where the backward's writes are ordered (`ordered`) - of their gradient rows; a zero cotangent gives exact zeros on
    every route"""
    n, res = LENGTHS[length]
    bits = ordered(res, n)
    case_id = f"isolation_{length}"
    x, y = draw(case_id, 3, 2, n)
    own = lambda t: torch.cat((t[0:2], t[4:6]))
    losses, grad = items_call(be, x, y, res, mr.SMOOTH, 3)
    assert torch.isfinite(losses).all() and torch.isfinite(grad).all()
    x2, y2 = draw(case_id + "_other", 3, 2, n)
    xo, yo = x.clone(), y.clone()
    xo[2:4], yo[2:4] = x2[2:4], y2[2:4]
    losses_o, grad_o = items_call(be, xo, yo, res, mr.SMOOTH, 3)
    assert losses_o[1] != losses[1]
    assert torch.equal(own(losses_o.repeat_interleave(2)), own(losses.repeat_interleave(2)))
    assert not bits or torch.equal(own(grad_o), own(grad))
    xn = x.clone()
    xn[2, n // 3] = float("nan")
    losses_n, grad_n = items_call(be, xn, y, res, mr.SMOOTH, 3)
    # The poisoned item's own value is whatever the scalar loss makes of its rows alone, bit for bit.  That is NOT NaN: the transform
    # kernels clamp |X|^2 with max(., eps), which drops a NaN operand, so mst_mrstft_forward returns a finite value for a prediction
    # holding NaN (or inf) on every route - and the per-item value is defined as that.
    alone = Call(be, xn[2:4], y[2:4], res, mr.SMOOTH).forward()
    assert same_bits(losses_n[1:2], alone), (losses_n[1], alone)
    assert torch.equal(own(losses_n.repeat_interleave(2)), own(losses.repeat_interleave(2)))
    assert not bits or torch.equal(own(grad_n), own(grad))
    losses_z, grad_z = items_call(be, x, y, res, mr.SMOOTH, 3, g=[1.0, 0.0, 1.0])
    assert torch.equal(losses_z, losses)
    assert torch.equal(grad_z[2:4], torch.zeros(2, n))
    assert not bits or torch.equal(own(grad_z), own(grad))


def check_cotangents(be, length):
    """g = (1, 2, 0.5): every item's gradient rows are its unit-cotangent rows times its own power of two, exactly (a route with
    an ordered backward: see `ordered`)"""
    n, res = LENGTHS[length]
    assert ordered(res, n)
    x, y = draw(f"cotangents_{length}", 3, 2, n)
    _, unit = items_call(be, x, y, res, mr.SMOOTH, 3)
    _, grad = items_call(be, x, y, res, mr.SMOOTH, 3, g=[1.0, 2.0, 0.5])
    assert torch.isfinite(unit).all()
    scale = torch.tensor([1.0, 1.0, 2.0, 2.0, 0.5, 0.5])[:, None]
    assert torch.equal(grad, unit * scale)


def check_mean_of_items_is_the_batch_loss(be, length):
    """sc_per_example and equal R: the float64 mean of the per-item values is the scalar loss up to one fp32 rounding on each side"""
    n, res = LENGTHS[length]
    x, y = draw(f"mean_{length}", 4, 2, n)
    c = Call(be, x, y, res, mr.SMOOTH)
    batch = c.forward().double().item()
    c.fresh()
    each = c.forward_items(4).double()
    bound = 2.0 ** -24 * (each.abs().max().item() + abs(batch))
    print(f"\n[mrstft items {length}] batch loss {batch:.9g}, mean of items {each.mean().item():.9g}, bound {bound:.3g}")
    assert abs(each.mean().item() - batch) <= bound


def check_beyond_staging(be, items):
    """five small resolutions at n = 1000, `items` stereo items: three sampled items graded; a second run gives the bits of the first
    in everything the reduction writes - the losses and the coefficient slab (the gradient of these generic resolutions is added by
    float atomics: see `ordered`)"""
    n, kw = 1000, mr.SMOOTH
    case_id = f"staging_{items}x2"
    x, y = draw(case_id, items, 2, n)
    c = Call(be, x, y, R5, kw)
    losses, grad = c.forward_items(items), c.backward_items(items, torch.ones(items))
    first = slabs(c, R5, n)
    grade_items(case_id, items, 2, n, R5, kw, losses, grad, which=(0, items // 2, items - 1))
    assert torch.isfinite(losses).all() and torch.isfinite(first.coef.view(-1, 4)[:, :3]).all()
    c.fresh()
    again = c.forward_items(items)
    assert same_bits(again, losses)
    assert same_bits(slabs(c, R5, n).coef, first.coef)
