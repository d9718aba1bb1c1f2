"""``TransformerController(graphed=True)`` (reference mst/modules.py:809-914): the hipGraph replay of the training-mode forward and
backward against the eager evaluation of the same module - same kernels, so the bound is rounding-level - over several calls
(static buffers reused), with and without the padding mask, and with the parameters updated in place between calls.

Second half of the file: the kernels of csrc/mst_ctrl.hip against torch's own ``nn.TransformerEncoder`` on the CPU in FLOAT64
(tests/ctrl_ref.py, shared with tests/test_ctrl_hostsim.py), graded three-way and by rel-L2 per tensor - h <= 3 r + F_GPU with h = the
kernels' distance from float64 and r = the fp32 CPU reference's - at the shapes the cases above never meet: partly populated upper
attention half, both sides of the dynamic-LDS cap, every feed-forward split, 16 layers, head widths 1 and 32, a non-default eps, the
``encoder_stack`` path and the torch-heads fallback.  Every such case passes the reference's ReLU-margin self-check first and asserts
that a repeated call is bit-identical ("No atomics: run-to-run deterministic")."""
import copy

import pytest
import torch

import ctrl_ref as R

pytestmark = pytest.mark.gpu


def _run(ctrl, te, me, mask, w):
    te = te.clone().requires_grad_(True)
    me = me.clone().requires_grad_(True)
    for p in ctrl.parameters():
        p.grad = None
    tp, fp, mp = ctrl(te, me, mask)
    loss = (tp * w[0]).sum() + (mp * w[2]).sum()  # the fx-bus output stays unused, as in the reference's configs
    loss.backward()
    return ([tp.detach().clone(), fp.detach().clone(), mp.detach().clone()], [te.grad.clone(), me.grad.clone()],
            {n: p.grad.clone() for n, p in ctrl.named_parameters() if p.grad is not None})


@pytest.mark.parametrize("with_mask", [False, True])
def test_graphed_controller_equals_eager(with_mask, record):
    from mst.modules import TransformerController

    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    ctrl = TransformerController(512, 27, 25, 26, num_layers=3, nhead=8, graphed=True, native=False).to(dev).train()
    keys = set(ctrl.state_dict().keys())
    bs, T = 2, 6
    worst = 0.0
    for it in range(3):
        te = torch.randn(bs, T, 512, device=dev)
        me = torch.randn(bs, 2, 512, device=dev)
        mask = None
        if with_mask:
            mask = torch.zeros(bs, T, dtype=torch.bool, device=dev)
            mask[0, T - 1 - it] = True
        w = [torch.randn(bs, T, 27, device=dev), None, torch.randn(bs, 26, device=dev)]
        ctrl.graphed = True
        out_g, gin_g, gp_g = _run(ctrl, te, me, mask, w)
        ctrl.graphed = False
        out_e, gin_e, gp_e = _run(ctrl, te, me, mask, w)
        assert set(gp_g) == set(gp_e) or set(gp_e) <= set(gp_g)
        for a, b in list(zip(out_g, out_e)) + list(zip(gin_g, gin_e)) + [(gp_g[n], gp_e[n]) for n in gp_e]:
            err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
            worst = max(worst, err)
            assert err <= 1e-5, err
        with torch.no_grad():  # an in-place optimizer step between replays: the graphs read the updated weights
            for p in ctrl.parameters():
                p.add_(0.01 * torch.randn_like(p))
    assert len(ctrl._graphs) == 1
    assert set(ctrl.state_dict().keys()) == keys  # the captured wrapper did not register itself under the controller
    record(max_rel_err=worst)


@pytest.mark.parametrize("bs,T,layers,with_mask,width,heads", [(2, 6, 2, True, 512, 8), (1, 32, 12, True, 512, 8), (3, 60, 2, False, 512, 8),
                                                               (2, 124, 1, True, 512, 8), (2, 9, 2, True, 256, 8), (1, 20, 1, True, 1024, 16),
                                                               (2, 5, 1, False, 128, 2)])
def test_native_encoder_stack_against_torch(bs, T, layers, with_mask, width, heads, record):
    """``TransformerController(native=True)``: the encoder stack on csrc/mst_ctrl.hip (fp32 MFMA) against torch's own
    ``nn.TransformerEncoder`` with the same weights - outputs, input gradients and every parameter gradient, fp32 tolerance
    (the reference's 1e-4); other widths / head counts than the reference's 512 / 8 cover the kernels' limits."""
    from mst.modules import TransformerController

    dev = torch.device("cuda:0")
    # seeds: 5 + bs + T, except the first case - with seed 13 one feed-forward unit of the last layer sits within rounding of
    # zero and its ReLU mask differs between the two fp32 evaluations (that unit's weight-gradient row moves by 9e-2 of the
    # largest entry with 20 rows in the batch; seeds 1-5 agree with float64 to 4e-7, tools/dbg_ctrl.py)
    torch.manual_seed(1 if (bs, T) == (2, 6) else 5 + bs + T)
    ctrl = TransformerController(width, 27, 25, 26, num_layers=layers, nhead=heads).to(dev).train()
    with torch.no_grad():  # LayerNorm / bias parameters off their 1 / 0 initial values
        for n, p in ctrl.named_parameters():
            if "norm" in n or n.endswith("bias"):
                p.add_(0.1 * torch.randn_like(p))
    te = torch.randn(bs, T, width, device=dev)
    me = torch.randn(bs, 2, width, device=dev)
    mask = None
    if with_mask:
        mask = torch.zeros(bs, T, dtype=torch.bool, device=dev)
        mask[0, T // 2:] = True
        mask[bs - 1, 1] = True
    w = [torch.randn(bs, T, 27, device=dev), None, torch.randn(bs, 26, device=dev)]
    ctrl.native = True
    out_n, gin_n, gp_n = _run(ctrl, te, me, mask, w)
    ctrl.native = False
    out_e, gin_e, gp_e = _run(ctrl, te, me, mask, w)
    worst_out = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(out_n, out_e))
    worst_gin = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gin_n, gin_e))
    worst_gp, worst_name = 0.0, ""
    assert set(gp_e) <= set(gp_n)
    for n in gp_e:
        err = float((gp_n[n] - gp_e[n]).abs().max() / gp_e[n].abs().max().clamp_min(1e-30))
        if err > worst_gp:
            worst_gp, worst_name = err, n
    record(out=worst_out, grad_in=worst_gin, grad_param=worst_gp)
    assert worst_out <= 1e-4, worst_out
    assert worst_gin <= 1e-4, worst_gin
    assert worst_gp <= 1e-4, (worst_name, worst_gp)


def test_native_controller_against_the_real_class(golden_dir, record):
    """Fixture from the REAL ``mst.modules.TransformerController`` (tests/golden/make_golden.py controller: seeded weights that the
    generator asserts equal to ours, padding mask, all three outputs weighted): outputs, input gradients, every parameter
    gradient of the HIP encoder stack within the reference's 1e-4."""
    import os

    import numpy as np
    from mst.modules import TransformerController
    from util import seeded_controller as _seeded_controller

    g = np.load(os.path.join(golden_dir, "controller_2x10.npz"))
    dev = torch.device("cuda:0")
    ctrl = _seeded_controller(TransformerController, int(g["seed_init"]), int(g["seed_pert"]), native=True).to(dev).train()
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    te, me = t("track_embeds").requires_grad_(True), t("mix_embeds").requires_grad_(True)
    tp, fp, mp = ctrl(te, me, t("mask"))
    ((tp * t("w_t")).sum() + (fp * t("w_f")).sum() + (mp * t("w_m")).sum()).backward()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    e_out = max(rel(tp.detach(), t("track_params")), rel(fp.detach(), t("fx_params")), rel(mp.detach(), t("master_params")))
    e_in = max(rel(te.grad, t("g_track_embeds")), rel(me.grad, t("g_mix_embeds")))
    e_par, worst = 0.0, ""
    for k, p in ctrl.named_parameters():
        if "g." + k in g.files:
            e = rel(p.grad, t("g." + k))
        else:
            e = max(rel(p.grad.flatten()[::499], t("gsub." + k)),
                    abs(float(p.grad.double().pow(2).sum().sqrt()) - float(g["gl2." + k])) / float(g["gl2." + k]))
        if e > e_par:
            e_par, worst = e, k
    record(out=e_out, grad_in=e_in, grad_param=e_par)
    assert e_out <= 1e-4 and e_in <= 1e-4, (e_out, e_in)
    assert e_par <= 1e-4, (worst, e_par)


def test_native_controller_limits_and_eval_mode():
    """Outside the kernels' limits ``native=True`` raises instead of silently running another path; inside, eval mode (no
    gradient) equals training mode (dropout is 0)."""
    from mst.modules import TransformerController

    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    ctrl = TransformerController(512, 27, 25, 26, num_layers=1, nhead=8, native=True).to(dev)
    te, me = torch.randn(1, 130, 512, device=dev), torch.randn(1, 2, 512, device=dev)  # 134 tokens > 128
    with pytest.raises(ValueError, match="limits"):
        ctrl(te, me)
    odd = TransformerController(192, 27, 25, 26, num_layers=1, nhead=8, native=True).to(dev)  # 192 % 128 != 0
    with pytest.raises(ValueError, match="limits"):
        odd(torch.randn(1, 4, 192, device=dev), torch.randn(1, 2, 192, device=dev))
    te, me = torch.randn(2, 7, 512, device=dev), torch.randn(2, 2, 512, device=dev)
    ctrl.train()
    a = ctrl(te, me)
    ctrl.eval()
    with torch.no_grad():
        b = ctrl(te, me)
    for x, y in zip(a, b):
        assert torch.equal(x.detach(), y)


# ---- float64 parity of csrc/mst_ctrl.hip --------------------------------------------------------------------------------------------------
# f of the bound h <= 3 r + f: 4x the largest h the cases below record on the MI355X, rounded up to one digit.
# Recorded maximum: 8.3e-7 (S = 127, where the fp32 reference itself sits 1.5e-6 from float64) -> 3.3e-6 -> 4e-6; every figure is in
# profiles/ctrl_parity.md.  The 16-layer case is left out of that maximum, which only makes f smaller: after 16 post-norm layers the
# tokens have all but collapsed onto each other, dQ and dK of the last layers are differences of nearly equal numbers, and on the Q / K
# thirds of their in_proj gradients BOTH fp32 evaluations sit at 1e-5 .. 7e-5 (h 2.6e-5, r 4.5e-5 at the worst tensor): that case is
# carried by 3 r, and a 4 x 2.6e-5 = 2e-4 would have loosened every other case fifty-fold.
F_GPU = 4e-6


@pytest.fixture(autouse=True)
def _cpu_threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))  # the float64 reference runs on the host


def _same(a, b, what):
    for k in ("out", "grad_tokens", "out_t", "out_f", "out_m", "grad_track_embeds", "grad_mix_embeds"):
        if k in a:
            assert torch.equal(a[k], b[k]), (what, k)
    assert set(a["grads"]) == set(b["grads"]), what
    for n in a["grads"]:
        assert torch.equal(a["grads"][n], b["grads"][n]), (what, n)


def _native_controller(ctrl, te, me, mask, g):
    """Forward and backward of a device controller -> a result shaped like ctrl_ref.controller_reference's, on the CPU."""
    dev = next(ctrl.parameters()).device
    for p in ctrl.parameters():
        p.grad = None
    te, me = te.to(dev).requires_grad_(True), me.to(dev).requires_grad_(True)
    outs = ctrl(te, me, None if mask is None else mask.to(dev))
    sum((o * w.to(dev)).sum() for o, w in zip(outs, g) if w is not None).backward()
    c = lambda t: t.detach().cpu()
    return dict(out_t=c(outs[0]), out_f=c(outs[1]), out_m=c(outs[2]), grad_track_embeds=c(te.grad), grad_mix_embeds=c(me.grad),
                grads={n: c(p.grad) for n, p in ctrl.named_parameters() if p.grad is not None})


def _native_stack(enc, tokens, mask, grad_out):
    from diffmst_hip import controller

    dev = next(enc.parameters()).device
    for p in enc.parameters():
        p.grad = None
    x = tokens.to(dev).requires_grad_(True)
    out = controller.encoder_stack(enc, x, None if mask is None else mask.to(dev))
    out.backward(grad_out.to(dev))
    c = lambda t: t.detach().cpu()
    return dict(out=c(out), grad_tokens=c(x.grad), grads={n: c(p.grad) for n, p in enc.named_parameters()})


def _controller(width, heads, n_heads, layers, ff):
    from mst.modules import TransformerController

    nt, nf, nm = n_heads
    ctrl = TransformerController(width, nt, nf, nm, num_layers=1 if ff != 2048 else layers, nhead=heads, native=True)
    if ff != 2048:  # the class fixes dim_feedforward at torch's default
        ctrl.transformer_encoder = R.make_encoder(width, heads, ff, layers)
    return R.perturb(ctrl).train()


def _check_controller(record, width, heads, n_heads, layers, ff, bs, T, masked=True, loss=(True, True, True)):
    dev = torch.device("cuda:0")
    nt, nf, nm = n_heads

    def build(seed):
        torch.manual_seed(seed)
        ctrl = _controller(width, heads, n_heads, layers, ff)
        te, me = torch.randn(bs, T, width), torch.randn(bs, 2, width)
        mask = R.padding_mask(bs, T) if masked else None
        g = [torch.randn(bs, T, nt), torch.randn(bs, nf), torch.randn(bs, nm)]
        g = tuple(w if on else None for w, on in zip(g, loss))
        return (ctrl, te, me, mask, g), R.controller_reference(ctrl, te, me, mask, *g)

    seed, case, ref = R.first_clean_seed(build)
    assert seed is not None, "no seed of ctrl_ref.SEEDS passes the reference's ReLU-margin self-check: resize the case"
    ctrl, te, me, mask, g = case
    ctrl = copy.deepcopy(ctrl).to(dev)
    got = _native_controller(ctrl, te, me, mask, g)
    _same(got, _native_controller(ctrl, te, me, mask, g), "repeated call")
    assert set(got["grads"]) == set(ref[torch.float64]["grads"])  # an unused head's projection reports None, like autograd
    h, r, _ = R.grade(got, ref, F_GPU, R.ROWS_CONTROLLER)
    record(h=h, r=r)
    return ctrl, case, got


def _check_stack(record, bs, S, d, heads, ff, layers, eps=1e-5):
    dev = torch.device("cuda:0")

    def build(seed):
        torch.manual_seed(seed)
        enc = R.perturb(R.make_encoder(d, heads, ff, layers, eps))
        tokens, grad_out = torch.randn(bs, S, d), torch.randn(bs, S, d)
        mask = R.padding_mask(bs, S)
        return (enc, tokens, mask, grad_out), R.stack_reference(enc, tokens, mask, grad_out)

    seed, case, ref = R.first_clean_seed(build)
    assert seed is not None, "no seed of ctrl_ref.SEEDS passes the reference's ReLU-margin self-check: resize the case"
    enc, tokens, mask, grad_out = case
    from diffmst_hip import controller

    enc = copy.deepcopy(enc).to(dev)
    assert controller.supported(enc, bs, S)
    got = _native_stack(enc, tokens, mask, grad_out)
    _same(got, _native_stack(enc, tokens, mask, grad_out), "repeated call")
    h, r, _ = R.grade(got, ref, F_GPU, R.ROWS_STACK)
    record(h=h, r=r)


@pytest.mark.parametrize("S", [65, 78, 79, 81, 82, 127])
def test_float64_parity_partial_upper_half_and_lds_cap(S, record):
    """Width 512, 8 heads, two layers, mask.  65 .. 127 tokens populate the `lane + 64 < S` half of the attention rows partly; the backward
    raises its dynamic-LDS cap from S = 79, the forward from S = 82.  (ff = 128 through a hand-built encoder: 2 x 127 x 2048 x 2 ReLU units
    would not leave the fp32 reference a clean margin; ff = 2048 runs at S = 128 in test_native_encoder_stack_against_torch.)"""
    _check_controller(record, 512, 8, (27, 25, 26), 2, 128, 2, S - 4)


def test_float64_parity_sixteen_layers_and_the_limit(record):
    """The documented limit of 16 layers (the batched weight-gradient launch carries 4 jobs per layer, 64 at the most); 17 raise."""
    _check_controller(record, 512, 8, (27, 25, 26), 16, 128, 2, 4)
    dev = torch.device("cuda:0")
    deep = _controller(512, 8, (27, 25, 26), 17, 128).to(dev)
    with pytest.raises(ValueError, match="limits"):
        deep(torch.randn(2, 4, 512, device=dev), torch.randn(2, 2, 512, device=dev))


@pytest.mark.parametrize("width,heads,T,ff", [(128, 2, 1, 2048), (1024, 16, 124, 128)])
def test_float64_parity_width_and_head_limits(width, heads, T, ff, record):
    """The narrowest and the widest model the kernels take, one track and 128 tokens, with head widths (1, 32, 32)."""
    _check_controller(record, width, heads, (1, 32, 32), 1, ff, 1 if T > 100 else 2, T)


@pytest.mark.parametrize("which", ["track", "master"])
def test_float64_parity_loss_on_one_head(which, record):
    """A loss on one head only: the other two heads hand None down, and their projections report None like autograd's."""
    loss = (which == "track", False, which == "master")
    _, _, got = _check_controller(record, 512, 8, (27, 25, 26), 1, 2048, 2, 6, loss=loss)
    unused = [n for n in ("track", "fx_bus", "master_bus") if not n.startswith(which)]
    for n in unused:
        assert f"{n}_projection.weight" not in got["grads"] and f"{n}_projection.bias" not in got["grads"]


def test_float64_parity_fallback_to_torch_heads(record):
    """40 > 32 head columns: the stack fits and the heads do not, so the call runs torch's token assembly, ``_EncoderStack`` and torch's
    heads - and meets the same bound."""
    from diffmst_hip import controller

    ctrl, _, _ = _check_controller(record, 512, 8, (40, 25, 26), 1, 2048, 2, 6)
    assert not controller.heads_supported(ctrl) and controller.supported(ctrl.transformer_encoder, 2, 10)


@pytest.mark.parametrize("bs,S,d,heads,ff,layers,eps", [
    (2, 9, 128, 2, 128, 2, 1e-5), (2, 9, 128, 2, 1024, 2, 1e-5), (2, 9, 128, 2, 1536, 1, 1e-5), (2, 9, 128, 2, 2560, 1, 1e-5),  # split_of 1, 2, 3, 1
    (2, 9, 384, 6, 128, 2, 1e-5), (2, 9, 640, 10, 128, 2, 1e-5),  # widths that are no power of two
    (2, 9, 128, 8, 128, 2, 1e-5),   # head width 16
    (2, 9, 128, 2, 128, 2, 1e-3),   # layer_norm_eps
    (40, 36, 128, 2, 128, 1, 1e-5),  # M = 1440: 23 row tiles
])
def test_float64_parity_encoder_stack(bs, S, d, heads, ff, layers, eps, record):
    """``controller.encoder_stack`` (the ``_EncoderStack`` node) on hand-built encoders."""
    _check_stack(record, bs, S, d, heads, ff, layers, eps)


def _outputs(ctrl, te, me, mask):
    te, me = te.clone().requires_grad_(True), me.clone().requires_grad_(True)
    for p in ctrl.parameters():
        p.grad = None
    outs = ctrl(te, me, mask)
    sum(o.sum() for o in outs).backward()
    return [o.detach() for o in outs] + [te.grad.float(), me.grad] + [p.grad for p in ctrl.parameters()]


def test_mask_dtypes_and_input_layouts_are_bit_identical():
    """The mask as uint8, int64 and float equals the bool mask bit for bit; ``track_embeds`` as a non-contiguous slice and as float64
    equals the contiguous fp32 call."""
    dev = torch.device("cuda:0")
    torch.manual_seed(R.SEEDS[0])
    bs, T = 2, 6
    ctrl = _controller(512, 8, (27, 25, 26), 2, 128).to(dev)
    te, me = torch.randn(bs, T, 512, device=dev), torch.randn(bs, 2, 512, device=dev)
    mask = R.padding_mask(bs, T).to(dev)
    want = _outputs(ctrl, te, me, mask)
    assert not any(bool(torch.isnan(t).any()) for t in want)
    for m in (mask.to(torch.uint8), mask.to(torch.int64), mask.float()):
        for a, b in zip(_outputs(ctrl, te, me, m), want):
            assert torch.equal(a, b), m.dtype
    wide = torch.randn(bs, 2 * T, 2 * 512, device=dev)
    wide[:, ::2, 512:] = te
    sliced = wide[:, ::2, 512:]
    assert not sliced.is_contiguous()
    for other in (sliced, te.double()):
        for a, b in zip(_outputs(ctrl, other, me, mask), want):
            assert torch.equal(a, b)


def test_masked_track_cannot_reach_the_other_tokens_on_the_device():
    """A masked key has probability exactly 0 in every layer: other finite values in a masked track's embedding leave every other
    output bit-identical (the masked track's own row may change)."""
    dev = torch.device("cuda:0")
    torch.manual_seed(R.SEEDS[0])
    bs, T = 2, 6
    ctrl = _controller(512, 8, (27, 25, 26), 2, 2048).to(dev)
    te, me = torch.randn(bs, T, 512, device=dev), torch.randn(bs, 2, 512, device=dev)
    mask = R.padding_mask(bs, T).to(dev)
    other = te.clone()
    other[mask] = 3.0 * torch.randn(int(mask.sum()), 512, device=dev) - 1.0
    with torch.no_grad():
        a, b = ctrl(te, me, mask), ctrl(other, me, mask)
    assert torch.equal(a[0][~mask], b[0][~mask]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not torch.equal(a[0][mask], b[0][mask])  # the replacement did reach the kernels
