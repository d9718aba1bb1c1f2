"""The reference of the controller tests (tests/test_ctrl_hostsim.py on the host simulator, tests/test_controller_gpu.py on the device):
torch's own ``nn.TransformerEncoder(enable_nested_tensor=False)`` - the computation the reference project runs (mst/modules.py:848-854) -
with the same weights on the CPU, evaluated in float64 AND in float32, plus the eager token assembly and head expressions of
``TransformerController._eager_forward``, and the three-way grading both test files share.

TEST INFRASTRUCTURE.  Three things are defined here once so that the two files cannot drift apart:

* ``stack_reference`` / ``controller_reference``: outputs, input gradients, every parameter gradient and the ReLU pre-activations of every
  layer (a forward hook on ``linear1``), per dtype.
* ``relu_margin_ok``: the self-check of a case.  One feed-forward unit whose pre-activation sits within rounding of zero flips its ReLU mask
  between two fp32 evaluations, and that moves everything upstream at the 1e-3 level - no kernel error, and no bound could tell the two
  apart.  A case is therefore only USED when no float64 pre-activation lies within 8x the largest |fp32 - float64| pre-activation
  difference of the CPU reference of zero: a margin taken from the reference, never from the kernels.  ``first_clean_seed`` walks a fixed
  sequence of 16 seeds and the test asserts that one was found (a condition on the construction, not a mask on the result).
* ``grade``: rel-L2 per tensor, h = kernels vs float64, r = fp32 CPU reference vs float64, asserted h <= 3 r + f.  ``in_proj_weight``'s
  gradient is graded by its Q, K and V thirds; ``in_proj_bias``'s as a whole (its K third is zero in exact arithmetic: softmax is invariant
  to a per-query constant, so it has no relative error of its own); tensors listed in ``rows`` also per token row, worst row taken, so that
  a whole-tensor norm cannot hide one padded row.
"""
import copy

import torch

SEEDS = tuple(range(101, 117))  # the fixed sequence a case draws its seed from
RELU_MARGIN = 8.0
SLACK = 3.0  # h <= SLACK * r + f


# ---- construction -----------------------------------------------------------------------------------------------------------------------
def make_encoder(d_model, nhead, d_ff, n_layers, eps=1e-5):
    """A hand-built stack of the reference's kind (post-norm, relu, dropout 0, batch_first, no final norm) with any d_ff / eps."""
    layer = torch.nn.TransformerEncoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=d_ff, dropout=0.0, batch_first=True,
                                             layer_norm_eps=eps)
    return torch.nn.TransformerEncoder(layer, num_layers=n_layers, enable_nested_tensor=False).train()


def perturb(module):
    """LayerNorm weights and every bias off their 1 / 0 initial values (a kernel that ignores one of them must not pass)."""
    with torch.no_grad():
        for n, p in module.named_parameters():
            if "norm" in n or n.endswith("bias"):
                p.add_(0.1 * torch.randn_like(p))
    return module


def padding_mask(bs, n, tail=True):
    """(bs, n) bool, True = padded key: the second half of example 0 and entry 1 of the last example (never a whole row of an example)."""
    mask = torch.zeros(bs, n, dtype=torch.bool)
    if n >= 2:
        if tail:
            mask[0, (n + 1) // 2:] = True
        mask[bs - 1, 1] = True
    return mask


def _torch_encoder(encoder, dtype):
    """A fresh ``nn.TransformerEncoder(enable_nested_tensor=False)`` with ``encoder``'s weights in ``dtype``."""
    l0 = encoder.layers[0]
    ref = make_encoder(l0.self_attn.embed_dim, l0.self_attn.num_heads, l0.linear1.out_features, len(encoder.layers), l0.norm1.eps)
    ref.load_state_dict({k: v.detach().cpu() for k, v in encoder.state_dict().items()})
    return ref.to(dtype)


def _hook_preacts(encoder, store):
    return [layer.linear1.register_forward_hook(lambda mod, inp, out: store.append(out.detach())) for layer in encoder.layers]


# ---- references -------------------------------------------------------------------------------------------------------------------------
def stack_reference(encoder, tokens, mask, grad_out):
    """-> {dtype: dict(out, grad_tokens, grads {name: tensor}, pre [per layer])} for float64 and float32, on the CPU."""
    res = {}
    for dtype in (torch.float64, torch.float32):
        ref = _torch_encoder(encoder, dtype)
        pre = []
        _hook_preacts(ref, pre)
        x = tokens.detach().cpu().to(dtype).requires_grad_(True)
        out = ref(x, src_key_padding_mask=None if mask is None else mask.cpu().bool())
        out.backward(grad_out.detach().cpu().to(dtype))
        res[dtype] = dict(out=out.detach(), grad_tokens=x.grad, grads={n: p.grad for n, p in ref.named_parameters()}, pre=pre)
    return res


def controller_reference(ctrl, track_embeds, mix_embeds, mask, g_t, g_f, g_m):
    """``TransformerController._eager_forward`` on torch's layers (the expressions of modules.py, not a restatement), both dtypes.
    g_* None = that output carries no loss.  -> {dtype: dict(out_t, out_f, out_m, grad_track_embeds, grad_mix_embeds, grads, pre)}."""
    res = {}
    for dtype in (torch.float64, torch.float32):
        ref = copy.deepcopy(ctrl).cpu()
        ref.native, ref.graphed = False, False
        ref.transformer_encoder = _torch_encoder(ctrl.transformer_encoder, dtype)
        ref = ref.to(dtype).train()
        pre = []
        _hook_preacts(ref.transformer_encoder, pre)
        te = track_embeds.detach().cpu().to(dtype).requires_grad_(True)
        me = mix_embeds.detach().cpu().to(dtype).requires_grad_(True)
        outs = ref._eager_forward(te, me, None if mask is None else mask.cpu().bool())
        loss = sum((o * g.detach().cpu().to(dtype)).sum() for o, g in zip(outs, (g_t, g_f, g_m)) if g is not None)
        loss.backward()
        res[dtype] = dict(out_t=outs[0].detach(), out_f=outs[1].detach(), out_m=outs[2].detach(), grad_track_embeds=te.grad,
                          grad_mix_embeds=me.grad, grads={n: p.grad for n, p in ref.named_parameters() if p.grad is not None}, pre=pre)
    return res


# ---- the self-check of a case -------------------------------------------------------------------------------------------------------------
def relu_margin(ref):
    """(smallest |float64 pre-activation|, largest |fp32 - float64| pre-activation difference) over every layer of a reference."""
    lo = min(float(p.abs().min()) for p in ref[torch.float64]["pre"])
    diff = max(float((a.double() - b).abs().max()) for a, b in zip(ref[torch.float32]["pre"], ref[torch.float64]["pre"]))
    return lo, diff


def relu_margin_ok(ref):
    lo, diff = relu_margin(ref)
    return lo > RELU_MARGIN * diff


def first_clean_seed(build):
    """``build(seed)`` -> (case, reference).  The first seed of SEEDS whose reference passes the self-check, or (None, None, None)."""
    for seed in SEEDS:
        case, ref = build(seed)
        if relu_margin_ok(ref):
            return seed, case, ref
    return None, None, None


# ---- grading ----------------------------------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    b = b.detach().double().cpu()
    den = float(b.norm())
    num = float((a.detach().double().cpu() - b).norm())
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den  # NaN (an element no kernel wrote) propagates and fails every comparison


def worst_row(a, b):
    """The largest rel-L2 over the rows (last axis = one row) of a tensor."""
    a2, b2 = a.detach().double().cpu().reshape(-1, a.shape[-1]), b.detach().double().cpu().reshape(-1, b.shape[-1])
    num, den = (a2 - b2).norm(dim=1), b2.norm(dim=1)
    rel = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf"))))
    if bool(torch.isnan(rel).any()):
        return float("nan")
    return float(rel.max())


def _pieces(name, t):
    if name.endswith("in_proj_weight"):
        d = t.shape[0] // 3
        return [(name + "[q]", t[:d]), (name + "[k]", t[d:2 * d]), (name + "[v]", t[2 * d:])]
    return [(name, t)]


def flatten(res, rows=()):
    """dict of a harness / reference result -> [(name, tensor, per_row)] of everything graded (``pre`` and non-tensors are skipped)."""
    out = []
    for k, v in res.items():
        if k == "grads":
            for n in sorted(v):
                out += [(pn, pt, False) for pn, pt in _pieces("grad " + n, v[n])]
        elif isinstance(v, torch.Tensor) and v.is_floating_point() and k in GRADED:
            out.append((k, v, False))
            if k in rows:
                out.append((k + " (worst row)", v, True))
    return out


GRADED = ("out", "grad_tokens", "out_t", "out_f", "out_m", "grad_track_embeds", "grad_mix_embeds")
ROWS_STACK = ("out", "grad_tokens")
ROWS_CONTROLLER = ("out_t", "grad_track_embeds", "grad_mix_embeds")


def grade(got, ref, f, rows=()):
    """Three-way grading of a result against ``ref`` ({float64: ..., float32: ...}).  Returns (worst h, worst r, table [(name, h, r)]) and
    raises AssertionError listing every tensor with h > 3 r + f (or a missing / NaN one).  What is graded is what the float64 reference
    holds: a projection whose head carried no loss has no gradient there, and the caller checks what the kernels did with it."""
    r64, r32 = ref[torch.float64], ref[torch.float32]
    g = {n: (t, pr) for n, t, pr in flatten(got, rows)}
    r = {n: t for n, t, _ in flatten(r32, rows)}
    table, bad = [], []
    for name, t64, per_row in flatten(r64, rows):
        if name not in g:
            bad.append((name, "missing"))
            continue
        m = worst_row if per_row else rel_l2
        h, rr = m(g[name][0], t64), m(r[name], t64)
        table.append((name, h, rr))
        if not h <= SLACK * rr + f:
            bad.append((name, h, rr))
    assert table, "nothing graded"
    assert not bad, f"h > {SLACK:g} r + {f:g} (name, h, r): {bad}"
    worst = max(table, key=lambda e: e[1])
    return worst[1], max(e[2] for e in table), table
