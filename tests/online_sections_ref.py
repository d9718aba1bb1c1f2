"""The shared cases of the pooled-sections tests: the pooled feature loss (tests/test_afpool_hostsim.py on the host simulator,
tests/test_afpool_gpu.py on the device) and the section-summing logit-Adam step (tests/test_online_sections_hostsim.py,
tests/test_online_sections_gpu.py).

TEST INFRASTRUCTURE.  Defined here once so that the simulator's and the device's files cannot drift apart.  The drivers, the guard
regions and the bounds are those of tests/afprofile_ref.py, tests/online_ref.py, tests/online_batch_ref.py and
tests/online_best_ref.py, imported unchanged:

* ``PoolDriver``: ``online_batch_ref.ItemsDriver`` plus ``mst_af_profile_pooled`` / ``mst_afloss_forward_profile_pooled`` /
  ``_backward_profile_pooled``.
* ``pooled_loss``: the pooled loss restated from ``oracle.loss_restated`` (its features of ``torch.cat(sections, dim=-1)``, its
  STFT and filterbank for the mean band energies over the sections), in whatever dtype the input has.
* ``SectionSession``: ``mst_logit_adam_init_sections`` / ``_step_sections`` on guarded buffers; ``online_ref.Session`` and
  ``online_best_ref.BestSession`` are the single sessions it is compared with, bit for bit.
"""
import ctypes
import functools
import os

import numpy as np
import torch

import afprofile_ref as A
import online_batch_ref as R
import online_best_ref as B
import online_ref as O
from oracle import loss_restated as ol
from util import rel

WEIGHTS = A.AF_WEIGHTS
NP = A.NP


# ================================================================ pooled feature loss ===============================================
class PoolDriver(R.ItemsDriver):
    def profile_pooled(self, x, items, sections):
        """x (items * sections, 2, n) host tensor -> (items, 54) float64 on the driver's device."""
        x = x.float().contiguous().to(self.device)
        bs, _, n = x.shape
        assert bs == items * sections
        nbytes = self.lib.mst_af_profile_workspace_bytes(bs, n)
        out = self.guarded(items * NP, torch.float64)
        self.lib.mst_af_profile_pooled(x, items, sections, n, self.tables, self.fb, out, self.workspace(nbytes), nbytes, self.stream_ptr())
        return out.view(items, NP)

    def loss_pooled(self, pred, profile, items, sections, weights, grad_losses=None):
        """pred (items * sections, 2, n) host tensor, profile (items, 54) on the device, grad_losses (items, 5) host tensor or None
        -> dict(losses (items, 5), grad_pred (items * sections, 2, n)) on the host."""
        x = pred.float().contiguous().to(self.device)
        bs, _, n = x.shape
        assert bs == items * sections and tuple(profile.shape) == (items, NP)
        nbytes = self.lib.mst_afloss_profile_workspace_bytes(bs, n)
        ws = self.workspace(nbytes)
        w = (ctypes.c_float * 5)(*weights)
        losses = self.guarded(items * 5)
        prof = profile.contiguous()
        self.lib.mst_afloss_forward_profile_pooled(x, prof, items, sections, n, w, self.tables, self.fb, losses, ws, nbytes,
                                                   self.stream_ptr())
        out = dict(losses=losses.view(items, 5).cpu().clone())
        if grad_losses is not None:
            g = grad_losses.float().contiguous().to(self.device)
            assert tuple(g.shape) == (items, 5)
            gx = self.guarded(x.numel())
            self.lib.mst_afloss_backward_profile_pooled(x, prof, items, sections, n, w, self.tables, self.fb, g, gx, ws, nbytes,
                                                        self.stream_ptr())
            out["grad_pred"] = gx.view_as(x).cpu().clone()
        if x.is_cuda:  # the upload: the isolation case's NaN does not go back to the allocator
            x.zero_()
        return out


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def lin_bark(x):
    """x (S, 2, n) -> (S, 24, 2) LINEAR band energies of mid and side, every row on its own: ``feat_barkspectrum`` before its log."""
    fb = ol.bark_filterbank(16385, 20.0, 20000.0, 24, 44100).to(x.dtype).t().unsqueeze(0)
    window = torch.hann_window(32768).to(x.dtype)
    outs = []
    for sig in (x[:, 0, :] + x[:, 1, :], x[:, 0, :] - x[:, 1, :]):
        X = torch.stft(sig, n_fft=32768, hop_length=8192, window=window, return_complex=True)
        outs.append(torch.matmul(fb, X.abs().mean(dim=-1, keepdim=True)))
    return torch.cat(outs, dim=-1)


def pooled_features(x):
    """The five features of the rows of x (S, 2, n) taken together, each in the shape the oracle gives a batch of one."""
    whole = torch.cat(list(x), dim=-1).unsqueeze(0)
    return dict(rms=ol.feat_rms(whole), crest_factor=ol.feat_crest_factor(whole), stereo_width=ol.feat_stereo_width(whole),
                stereo_imbalance=ol.feat_stereo_imbalance(whole),
                barkspectrum=torch.log(lin_bark(x).mean(dim=0, keepdim=True) + 1e-8))


def target_features(y):
    """The oracle's five features of a target y (1, 2, m)."""
    return {name: fn(y) for name, fn in A.FEATS}


def pooled_loss(x, y, weights):
    """The five weighted terms of sections x (S, 2, n) against a target y (1, 2, m), in x's dtype."""
    fx, fy = pooled_features(x), target_features(y.to(x.dtype))
    return torch.stack([w * torch.nn.functional.mse_loss(fx[name], fy[name]) for w, (name, _) in zip(weights, A.FEATS)])


def sections_audio(items, sections, n, m, seed=0):
    """Correlated-channel noise without peak ties, section s scaled by 0.5 (1 + s): the pooled peak sits in the last section and
    pooling is distinguishable from averaging features.  -> x (items * sections, 2, n), y (items, 2, m)."""
    g = torch.Generator().manual_seed(9000 + 131 * items + 17 * sections + n + seed)
    x = 0.2 * torch.randn(items * sections, 2, n, generator=g)
    x[:, 1] = 0.6 * x[:, 1] + 0.3 * x[:, 0]
    scale = 0.5 * (1.0 + torch.arange(sections, dtype=torch.float32)).repeat(items)
    x = x * scale.view(-1, 1, 1)
    y = 0.3 * torch.randn(items, 2, m, generator=g) * torch.tensor([1.0, 0.5]).view(1, 2, 1)
    return x, y


@functools.lru_cache(maxsize=None)
def references(items, sections, n, m):
    """(x, y, [per item {dtype: (five losses as float64, gradient (S, 2, n))}]): computed once, shared, never modified.  The premise
    of the three-way bound is checked here, on the host: the fp32 restatement is finite, no feature is clamped and no two section
    peaks of a channel lie within 1e-3 of each other (a tie the fp32 and float64 evaluations could break differently)."""
    x, y = sections_audio(items, sections, n, m)
    gw = torch.tensor(A.COTANGENT)
    res = []
    for item in range(items):
        xs, per = x[item * sections:(item + 1) * sections], {}
        peaks = xs.abs().amax(dim=-1).double()  # (S, 2)
        for ch in range(2):
            p = peaks[:, ch].sort().values
            assert bool(((p[1:] - p[:-1]) / p[1:] > 1e-3).all()), "two section peaks too close"
        whole = torch.cat(list(xs), dim=-1)
        assert float(whole.pow(2).mean(dim=-1).min()) > 1e-6 and float((whole[0] + whole[1]).pow(2).mean()) > 1e-6  # no clamp is active
        for dt in (torch.float32, torch.float64):
            xo = xs.clone().to(dt).requires_grad_(True)
            vo = pooled_loss(xo, y[item:item + 1], WEIGHTS)
            (vo * gw.to(dt)).sum().backward()
            assert bool(torch.isfinite(vo).all()) and bool(torch.isfinite(xo.grad).all())
            per[dt] = (vo.detach().double(), xo.grad)
        res.append(per)
    return x, y, res


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
_RUNS = {}  # (device, case) -> what a case computed: shared by the cases that start from it, never modified


def single_run(drv, n, m):
    """(x (1, 2, n), profile of y, cotangent (1, 5), the pooled call at items = 1, sections = 1)."""
    key = (drv.device.type, "single", n, m)
    if key not in _RUNS:
        x, y = R.audio(1, n, m, seed=3)
        prof, g = drv.profile(y).clone(), torch.tensor([A.COTANGENT])  # a copy of its own: a driver's buffers may be scrubbed after a test
        one = drv.loss_pooled(x, prof, 1, 1, WEIGHTS, g)
        drv.check_guards()
        assert bool(torch.isfinite(one["losses"]).all()) and bool(torch.isfinite(one["grad_pred"]).all()), "an output element was not written"
        _RUNS[key] = (x, y, prof, g, one)
    return _RUNS[key]


def pooled_run(drv, items, sections, n, m):
    """(x, profile of y, cotangent (items, 5), the pooled call) on the inputs of ``references``."""
    key = (drv.device.type, "pooled", items, sections, n, m)
    if key not in _RUNS:
        x, y, _ = references(items, sections, n, m)
        prof, g = drv.profile(y).clone(), torch.tensor(A.COTANGENT).expand(items, 5)  # a copy of its own, as above
        got = drv.loss_pooled(x, prof, items, sections, WEIGHTS, g)
        drv.check_guards()  # exactly items * 5 losses and bs * 2 * n gradient elements between untouched guards
        assert bool(torch.isfinite(got["losses"]).all()) and bool(torch.isfinite(got["grad_pred"]).all()), "an output element was not written"
        _RUNS[key] = (x, prof, g, got)
    return _RUNS[key]


def check_one_section_is_the_items_call(drv, n, m):
    """Check 1: sections = 1 is mst_afloss_forward_profile_items / _backward_profile_items / mst_af_profile, bit for bit."""
    x, y, prof, g, pooled = single_run(drv, n, m)
    assert torch.equal(A.bits(drv.profile_pooled(y, 1, 1)), A.bits(prof))
    items = drv.loss_items(x, prof, WEIGHTS, g)
    drv.check_guards()
    assert torch.equal(A.bits(pooled["losses"]), A.bits(items["losses"]))
    assert torch.equal(A.bits(pooled["grad_pred"]), A.bits(items["grad_pred"]))


def check_pooled_three_way(drv, items, sections, n, m, record=None):
    """Check 2: every item against the float64 restatement, with afprofile_ref's three-way bound (its factor, its floor)."""
    x, _, res = references(items, sections, n, m)
    got = pooled_run(drv, items, sections, n, m)[3]
    triples = {}
    for item in range(items):
        rows = slice(item * sections, (item + 1) * sections)
        A.assert_three_way(f"pooled item {item} of {items}x{sections}x2x{n} vs {m}", got["losses"][item], got["grad_pred"][rows], res[item],
                           None if record is None else lambda item=item, **values: triples.update({f"item{item}_{k}": v for k, v in values.items()}))
    if record is not None:
        record(**triples)
    # pooling is not averaging: the peak of the whole sits in the last section, and only there does the crest delta land
    for item in range(items):
        xs = x[item * sections:(item + 1) * sections]
        assert int(xs.abs().amax(dim=-1)[:, 0].argmax()) == sections - 1


def check_copies(drv, n, m, copies=(2, 4)):
    """Check 3: S copies of one section.  The losses are the S = 1 call's bits; away from the two arg-max samples S * grad_s is the
    S = 1 gradient's bits for every section; the crest delta appears in section 0 only - the tie rule."""
    x, _, prof, g, one = single_run(drv, n, m)
    at = [int(x[0, ch].abs().argmax()) for ch in range(2)]
    for S in copies:
        got = drv.loss_pooled(x.repeat(S, 1, 1), prof, 1, S, WEIGHTS, g)
        drv.check_guards()
        assert torch.equal(A.bits(got["losses"]), A.bits(one["losses"])), f"S = {S}: the losses of {S} copies differ from one"
        scaled = float(S) * got["grad_pred"]
        away = torch.ones(2, n, dtype=torch.bool)
        for ch in range(2):
            away[ch, at[ch]] = False
        for s in range(S):
            assert torch.equal(A.bits(scaled[s][away]), A.bits(one["grad_pred"][0][away])), f"S = {S}, section {s}"
        for s in range(2, S):
            assert torch.equal(A.bits(got["grad_pred"][s]), A.bits(got["grad_pred"][1])), "later sections differ among themselves"
        for ch in range(2):
            four = [float(v) for v in (got["grad_pred"][0, ch, at[ch]], got["grad_pred"][1, ch, at[ch]], one["grad_pred"][0, ch, at[ch]],
                                       scaled[1, ch, at[ch]])]
            d0, d1 = four[0] - four[1], four[2] - four[3]  # the delta: in section 0 only, and the S = 1 call's
            # each of the four is one fp32 sum of the delta and the (exactly scaled) rest: they differ by roundings of those sums
            assert d1 != 0.0 and abs(d0 - d1) <= 2.0 ** -21 * max(abs(v) for v in four), (S, ch, d0, d1)


def check_golden(drv, record=None):
    """Check 4: profile(x, pool=True)'s five views against what the reference's own functions returned (af_pooled.npz): its
    compute_rms ... compute_stereo_imbalance of the concatenation, its compute_barkspectrum of every section pooled in float64 by
    log(mean_s(exp(B_s) - 1e-8) + 1e-8); rel(hip, f64) <= 3 rel(fixture, f64) + 2e-5 with the float64 restatement as truth."""
    g = np.load(os.path.join(A.GOLDEN, "af_pooled.npz"))
    x = torch.from_numpy(g["sections"])
    got = A.views(A.profile_object(drv.profile_pooled(x, 1, x.shape[0])))
    drv.check_guards()  # exactly 54 doubles
    bark = torch.from_numpy(g["feat.bark_sections"]).double()
    fixture = {name: torch.from_numpy(g["feat." + key]).double() for (name, _), key in zip(A.FEATS[:4], ("rms", "crest", "width", "imbalance"))}
    fixture["barkspectrum"] = torch.log((torch.exp(bark) - 1e-8).mean(dim=0, keepdim=True) + 1e-8)
    truth = pooled_features(x.double())
    for name, _ in A.FEATS:
        assert got[name].shape == truth[name].shape == fixture[name].shape, (name, got[name].shape, truth[name].shape, fixture[name].shape)
        e, e_fix = rel(got[name], truth[name]), rel(fixture[name], truth[name])
        print(f"[af pooled golden] {name}: hip-f64 {e:.2e}  fixture-f64 {e_fix:.2e}")
        if record is not None:
            record(**{name: (e, e_fix)})
        assert e <= 3 * e_fix + 2e-5, (name, e, e_fix)


def check_known_answers(drv, n=20000, noise=True, zero=True):
    """Check 5: sections against their own pooled profile give exactly 0; a loud and a silent section of a +-1 square wave pool to
    rms sqrt(1/2) and crest factor 20 log10(sqrt 2).  ``noise``: the zero also on two items of three sections of noise."""
    sq = torch.ones(2, 2, n)
    sq[..., ::2] = -1.0  # +-1 square wave: every sum of squares is exact
    sq[1] = 0.0
    own = drv.profile_pooled(sq, 1, 2)
    p = A.profile_object(own)
    assert bool((p.rms.cpu() - 0.5 ** 0.5).abs().max() < 1e-6)
    assert bool((p.crest_factor.cpu() - 20.0 * np.log10(2.0 ** 0.5)).abs().max() < 1e-5)
    if zero:
        z = drv.loss_pooled(sq, own, 1, 2, [1.0] * 5)["losses"]
        assert bool((z == 0).all()), z.tolist()
    if noise:
        x, _ = sections_audio(2, 3, n, n)
        z = drv.loss_pooled(x, drv.profile_pooled(x, 2, 3), 2, 3, [1.0] * 5)["losses"]
        assert bool((z == 0).all()), z.tolist()
    drv.check_guards()


def check_isolation(drv, n, m):
    """Check 6 (and a second run of item 0, check 7): a NaN in item 1 leaves item 0's losses and gradient bit-equal."""
    items, sections = 2, 2
    x, prof, g, base = pooled_run(drv, items, sections, n, m)
    bad = x.clone()
    bad[3, 0, n // 3] = float("nan")  # section 1 of item 1
    out = drv.loss_pooled(bad, prof, items, sections, WEIGHTS, g)
    drv.check_guards()
    assert bool(torch.isnan(out["losses"][1]).any()), "the NaN did not reach its own item"
    assert torch.equal(A.bits(out["losses"][0]), A.bits(base["losses"][0]))
    assert torch.equal(A.bits(out["grad_pred"][:sections]), A.bits(base["grad_pred"][:sections]))


def check_reproducible(drv, items, sections, n, m):
    """Checks 7 and 8: a second run gives the same bits, in the loss, the gradient and the pooled profile; exactly items * 5 losses,
    items * 54 doubles and bs * 2 * n gradient elements are written between untouched guards."""
    x, prof, g, base = pooled_run(drv, items, sections, n, m)
    again = drv.loss_pooled(x, prof, items, sections, WEIGHTS, g)
    profiles = [drv.profile_pooled(x, items, sections).cpu().clone() for _ in range(2)]
    drv.check_guards()
    assert bool(torch.isfinite(profiles[0]).all()), "profile not fully written"
    assert torch.equal(A.bits(profiles[0]), A.bits(profiles[1]))
    assert torch.equal(A.bits(again["losses"]), A.bits(base["losses"])) and torch.equal(A.bits(again["grad_pred"]), A.bits(base["grad_pred"]))


def check_pooled_refusals(drv):
    """Check 9: every refusal returns non-zero and writes nothing."""
    from mst import _cabi

    L, st = drv.lib, drv.stream_ptr()
    for name in ("mst_af_profile_pooled", "mst_afloss_forward_profile_pooled", "mst_afloss_backward_profile_pooled"):
        assert hasattr(L, name) and name in _cabi.SIGNATURES
    assert L.mst_abi_version() == _cabi.ABI_VERSION == 13
    items, S, n = 1, 2, 17000
    bs = items * S
    xd = torch.zeros(bs, 2, n, device=drv.device)
    prof, losses, gx = drv.guarded(items * NP, torch.float64), drv.guarded(items * 5), drv.guarded(bs * 2 * n)
    g = torch.ones(items, 5, device=drv.device)
    w = (ctypes.c_float * 5)(*WEIGHTS)
    nb_p, nb = L.mst_af_profile_workspace_bytes(bs, n), L.mst_afloss_profile_workspace_bytes(bs, n)
    ws = drv.workspace(nb)

    def refused(fn, *args):
        try:
            fn(*args)
        except _cabi.AbiError as e:
            assert e.code != 0
            return
        raise AssertionError(f"{fn.__name__} accepted {args}")

    good = dict(x=xd, items=items, S=S, n=n, tables=drv.tables, fb=drv.fb, prof=prof, ws=ws, w=w, losses=losses, g=g, gx=gx, nb=nb, nb_p=nb_p)
    common = (dict(n=16384), dict(items=0), dict(items=-1), dict(S=0), dict(S=-3), dict(x=None), dict(tables=None), dict(fb=None),
              dict(prof=None), dict(ws=None))
    for change in common + (dict(nb_p=nb_p - 4),):
        a = dict(good, **change)
        refused(L.mst_af_profile_pooled, a["x"], a["items"], a["S"], a["n"], a["tables"], a["fb"], a["prof"], a["ws"], a["nb_p"], st)
    for change in common + (dict(w=None), dict(losses=None), dict(nb=nb - 4)):
        a = dict(good, **change)
        refused(L.mst_afloss_forward_profile_pooled, a["x"], a["prof"], a["items"], a["S"], a["n"], a["w"], a["tables"], a["fb"],
                a["losses"], a["ws"], a["nb"], st)
    for change in common + (dict(w=None), dict(g=None), dict(gx=None), dict(nb=nb - 4)):
        a = dict(good, **change)
        refused(L.mst_afloss_backward_profile_pooled, a["x"], a["prof"], a["items"], a["S"], a["n"], a["w"], a["tables"], a["fb"], a["g"],
                a["gx"], a["ws"], a["nb"], st)
    for t in (prof, losses, gx, ws):
        assert bool(torch.isnan(t).all()), "a refused call wrote something"
    drv.check_guards()


# ================================================================ section-summing logit-Adam ======================================
class SectionSession:
    """One optimiser state over segments that start at ``theta0`` (host tensors); p has ``sections`` rows per segment.  ``best``: with
    a zero-filled best block, as ``online_best_ref.BestSession``."""

    def __init__(self, drv, theta0, sections, n_iters, n_terms, best=False):
        from mst import _cabi

        self.drv, self.cabi, self.sections = drv, _cabi, sections
        self.counts = [t.numel() for t in theta0]
        self.n = sum(self.counts)
        self.theta = [drv.guarded(c) for c in self.counts]
        for dst, src in zip(self.theta, theta0):
            dst.copy_(src)
        self.p = [drv.guarded(sections * c) for c in self.counts]
        nbytes = drv.lib.mst_logit_adam_state_bytes(self.n)
        self.state = drv.guarded(nbytes // 4).view(torch.int32)
        self.history = drv.guarded(n_iters * (1 + n_terms)).view(n_iters, 1 + n_terms)
        self.best = B._zeroed_best(drv, drv.lib.mst_logit_adam_best_bytes(1, self.n) // 4) if best else None
        self.n_terms, self.calls = n_terms, 0
        drv.lib.mst_logit_adam_init_sections(self._segments([None] * len(theta0)), len(theta0), sections, self.state, drv.stream_ptr())
        assert not bool(self.state.cpu().any()), "state not zeroed"

    def _segments(self, grads):
        seg = (self.cabi.LogitAdamSegment * len(self.counts))()
        for s, th, p, g, c in zip(seg, self.theta, self.p, grads, self.counts):
            s.theta, s.p, s.grad_p, s.count = th.data_ptr(), p.data_ptr(), None if g is None else g.data_ptr(), c
        return seg

    def step(self, grads, terms, lr, min_delta=0.0, patience=0, betas=O.BETAS, eps=O.EPS):
        """grads: per segment a (sections, count) fp32 tensor on the driver's device or None; terms: (n_terms,) fp32 there."""
        assert terms.numel() == self.n_terms
        for g, c in zip(grads, self.counts):
            assert g is None or (tuple(g.shape) == (self.sections, c) and g.is_contiguous())
        ptrs = (ctypes.c_void_p * self.n_terms)(*[terms.data_ptr() + 4 * j for j in range(self.n_terms)])
        self.drv.lib.mst_logit_adam_step_sections(self._segments(grads), len(self.counts), self.sections, ptrs, self.n_terms,
                                                  self.history[self.calls], lr, betas[0], betas[1], eps, min_delta, patience, self.state,
                                                  self.best, self.drv.stream_ptr())
        self.calls += 1

    def words(self):
        return tuple(self.state[:4].cpu().tolist())

    def rows(self, s):
        return self.p[s].view(self.sections, self.counts[s])


def host_sum(g):
    """g (S, count) host fp32 -> ((g[0] + g[1]) + g[2]) + ..., one IEEE fp32 addition at a time."""
    acc = g[0].clone()
    for r in range(1, g.shape[0]):
        acc = acc + g[r]
    return acc


def section_streams(counts, steps, sections, seed=100):
    """Per segment a (steps, sections, count) host stream of gradients: ``sections`` independent ``online_ref.gradient_stream`` draws."""
    draws = [O.gradient_stream(counts, steps, seed + r)[0] for r in range(sections)]
    return [torch.stack([draws[r][s] for r in range(sections)], dim=1).contiguous() for s in range(len(counts))]


def assert_same_as_single(ses, one, tag):
    """theta, every p row, the whole state block (header and moments), the history rows written so far, the best block."""
    for s, (a, b) in enumerate(zip(ses.theta, one.theta)):
        assert B.same(a, b), f"{tag}: theta of segment {s} differs from the single session"
    for s, b in enumerate(one.p):
        for r in range(ses.sections):
            assert B.same(ses.rows(s)[r], b), f"{tag}: row {r} of p of segment {s} differs from the single session's p"
    assert torch.equal(ses.state.cpu(), one.state.cpu()), f"{tag}: state words or moments differ"
    assert B.same(ses.history[:ses.calls], one.history[:one.calls]), f"{tag}: history differs"
    if ses.best is not None:
        assert torch.equal(ses.best.cpu(), one.best.cpu()), f"{tag}: best block differs"


def check_one_section_is_the_single_step(drv, name, best, steps=50):
    """Check 10: sections = 1 against mst_logit_adam_step / _step_best, bit for bit after every step."""
    counts, _, lr, scale = O.STREAMS[name]
    theta0 = O.start(counts, scale, 0)
    stream, _, _ = O.gradient_stream(counts, steps, 0)
    terms = torch.rand(steps, 2, generator=torch.Generator().manual_seed(41)) + 0.5
    dev = drv.device
    one = (B.BestSession if best else O.Session)(drv, theta0, steps, 2)
    ses = SectionSession(drv, theta0, 1, steps, 2, best=best)
    up, tm = [s.to(dev).contiguous() for s in stream], terms.to(dev).contiguous()
    extra = (0.01, 4) if best else ()
    for k in range(steps):
        one.step([s[k] for s in up], tm[k], lr, *extra)
        ses.step([s[k:k + 1] for s in up], tm[k], lr, *extra)
        if k % 7 == 0 or k == steps - 1:  # a difference never heals: theta, the moments and the history carry it to the last step
            assert_same_as_single(ses, one, f"{name} step {k}")
    drv.check_guards()
    if not best:
        assert ses.words() == (steps, 0, 0, steps)


def check_sum_of_sections(drv, sections, counts, steps, lr, scale):
    """Check 11: bit for bit a single mst_logit_adam_step session fed g[0] + g[1] + ... formed sequentially in fp32 on the host; every
    p row equals that session's p."""
    theta0 = O.start(counts, scale, 7)
    streams = section_streams(counts, steps, sections)
    summed = [torch.stack([host_sum(s[k]) for k in range(steps)]) for s in streams]
    terms = torch.rand(steps, 1, generator=torch.Generator().manual_seed(43)) + 0.5
    dev = drv.device
    one = O.Session(drv, theta0, steps, 1)
    ses = SectionSession(drv, theta0, sections, steps, 1)
    up, us, tm = [s.to(dev) for s in streams], [s.to(dev) for s in summed], terms.to(dev)
    for k in range(steps):
        one.step([s[k] for s in us], tm[k], lr)
        ses.step([s[k] for s in up], tm[k], lr)
        if k % 7 == 0 or k == steps - 1:
            assert_same_as_single(ses, one, f"{sections} sections of {counts}, step {k}")
    drv.check_guards()
    assert ses.words() == (steps, 0, 0, steps)


def check_sections_nonfinite(drv, where, at=3, steps=6):
    """Check 12: a NaN in one section's gradient, or two finite addends whose sum overflows, at step 3 of 6: that step changes
    nothing and is the one reported."""
    counts, lr, sections = O.STREAMS["song3"][0], 1e-3, 3
    theta0 = O.start(counts, 1e-3, 9)
    streams = [s.clone() for s in section_streams(counts, steps, sections, seed=200)]
    if where == "nan":
        streams[2][at, 1, 7] = float("nan")
    else:
        streams[0][at, 0, 5] = 3e38
        streams[0][at, 1, 5] = 3e38
        assert bool(torch.isfinite(streams[0][at]).all()) and not bool(torch.isfinite(host_sum(streams[0][at])).all())
    terms = torch.rand(steps, 2, generator=torch.Generator().manual_seed(44))
    dev = drv.device
    ses = SectionSession(drv, theta0, sections, steps, 2)
    snaps = []
    for k in range(steps):
        ses.step([s[k].to(dev).contiguous() for s in streams], terms[k].to(dev), lr)
        snaps.append((torch.cat([t.cpu() for t in ses.theta]), ses.state.cpu().clone()[O.HDR:], torch.cat([p.cpu() for p in ses.p])))
    drv.check_guards()
    for a, b in zip(snaps[at], snaps[at - 1]):
        assert B.same(a, b), "the rejected step changed theta, the moments or p"
    assert not B.same(snaps[at + 1][0], snaps[at][0]), "the step after it did not move"
    assert bool(torch.isfinite(snaps[-1][0]).all())
    assert ses.words() == (steps - 1, 1, at, steps)
    h = ses.history.cpu()
    assert torch.equal(O.bits(h[:, 1:]), O.bits(terms)), "a history row was not written"


def check_sections_null_gradient(drv):
    """Check 13: a NULL-gradient segment keeps theta, its moments and every row of p bit for bit."""
    counts, lr, sections, steps = O.STREAMS["song3"][0], 1e-3, 3, 10
    theta0 = O.start(counts, 1e-3, 11)
    streams = section_streams(counts, steps, sections, seed=300)
    dev = drv.device
    ses = SectionSession(drv, theta0, sections, steps, 1)
    p0 = ses.p[1].clone()
    term = torch.ones(1, device=dev)
    for k in range(steps):
        ses.step([None if s == 1 else g[k].to(dev).contiguous() for s, g in enumerate(streams)], term, lr)
    drv.check_guards()
    assert B.same(ses.theta[1], theta0[1].to(dev)) and B.same(ses.p[1], p0)
    for r in range(sections):
        assert B.same(ses.rows(1)[r], ses.rows(1)[0])
    st = ses.state.cpu()
    lo, hi = counts[0], counts[0] + counts[1]
    m, v = st[O.HDR:O.HDR + ses.n], st[O.HDR + ses.n:]
    assert not bool(m[lo:hi].any()) and not bool(v[lo:hi].any()) and bool(m[:lo].any()) and bool(v[hi:].any())
    assert ses.words() == (steps, 0, 0, steps)


def check_sections_refusals(drv):
    """Check 14: sections 0 and 65, NULL pointers and the single call's hyper-parameter cases launch nothing."""
    from mst import _cabi

    L, st = drv.lib, drv.stream_ptr()
    for name in ("mst_logit_adam_init_sections", "mst_logit_adam_step_sections"):
        assert hasattr(L, name) and name in _cabi.SIGNATURES
    sections = 2
    theta, row, term = drv.guarded(8), drv.guarded(8), drv.guarded(8)
    p, grad = drv.guarded(sections * 8), drv.guarded(sections * 8)
    state, best = drv.guarded(O.HDR + 2 * 8), drv.guarded(B.best_words(8))
    seg = (_cabi.LogitAdamSegment * 1)()
    seg[0].theta, seg[0].p, seg[0].grad_p, seg[0].count = theta.data_ptr(), p.data_ptr(), grad.data_ptr(), 8
    ptrs = (ctypes.c_void_p * 1)(term.data_ptr())

    def refused(fn, *args):
        try:
            fn(*args)
        except _cabi.AbiError as e:
            assert e.code != 0
            return
        raise AssertionError(f"{fn.__name__} accepted {args}")

    good = dict(n_seg=1, S=sections, ptrs=ptrs, n_terms=1, row=row, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, delta=0.0, patience=0,
                state=state, best=None)
    for change in (dict(S=0), dict(S=65), dict(S=-1), dict(n_seg=0), dict(n_seg=5), dict(ptrs=None), dict(n_terms=0), dict(n_terms=9),
                   dict(row=None), dict(state=None), dict(lr=0.0), dict(lr=float("nan")), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0),
                   dict(best=best, delta=-1e-3), dict(best=best, delta=float("nan")), dict(best=best, patience=-1),
                   dict(best=best.data_ptr() + 2)):
        a = dict(good, **change)
        refused(L.mst_logit_adam_step_sections, seg, a["n_seg"], a["S"], a["ptrs"], a["n_terms"], a["row"], a["lr"], a["b1"], a["b2"],
                a["eps"], a["delta"], a["patience"], a["state"], a["best"], st)
    for bad in (0, 65):
        refused(L.mst_logit_adam_init_sections, seg, 1, bad, state, st)
    refused(L.mst_logit_adam_init_sections, seg, 1, sections, None, st)
    refused(L.mst_logit_adam_init_sections, None, 1, sections, state, st)
    seg[0].p = None
    refused(L.mst_logit_adam_init_sections, seg, 1, sections, state, st)
    refused(L.mst_logit_adam_step_sections, seg, 1, sections, ptrs, 1, row, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, state, None, st)
    for t in (theta, p, grad, row, term, state, best):
        assert bool(torch.isnan(t).all()), "a refused call wrote something"
    drv.check_guards()


def check_sections_best(drv, sections=3):
    """Check 15: online_best_ref's hand-worked loss sequence gives the single kernel's verdicts - and its bits - on summed gradients."""
    counts, steps = B.COUNTS, len(B.SEQUENCE)
    theta0 = O.start(counts, 1e-3, 11)
    streams = section_streams(counts, steps, sections, seed=400)
    summed = [torch.stack([host_sum(s[k]) for k in range(steps)]) for s in streams]
    dev = drv.device
    one = B.BestSession(drv, theta0, steps, 1)
    ses = SectionSession(drv, theta0, sections, steps, 1, best=True)
    terms = torch.tensor(B.SEQUENCE, dtype=torch.float32).view(steps, 1).to(dev)
    up, us = [s.to(dev) for s in streams], [s.to(dev) for s in summed]
    for k in range(steps):
        one.step([s[k] for s in us], terms[k], B.LR, 0.25, 3)
        ses.step([s[k] for s in up], terms[k], B.LR, 0.25, 3)
        assert_same_as_single(ses, one, f"best, step {k}")
    drv.check_guards()
    assert one.header() == (4 + 1, 2.5, 3, 7 + 1)  # the figures online_best_ref works by hand
    assert tuple(ses.best[:4].cpu().tolist()) == tuple(one.best[:4].cpu().tolist())
    assert ses.words() == (8, 0, 0, 10)
