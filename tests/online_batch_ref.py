"""The shared cases of the batched-fit tests: the per-item feature loss (tests/test_afitems_hostsim.py on the host simulator,
tests/test_afitems_gpu.py on the device) and the batched logit-Adam step (tests/test_online_batch_hostsim.py, tests/test_online_batch_gpu.py).

TEST INFRASTRUCTURE.  Defined here once so that the simulator's and the device's files cannot drift apart.  The drivers, the guard
regions, the oracle and the bounds are those of tests/afprofile_ref.py and tests/online_ref.py, imported unchanged:

* ``ItemsDriver``: ``afprofile_ref.Driver`` plus ``mst_afloss_forward_profile_items`` / ``_backward_profile_items``.
* ``pair``: the per-item call and the batch call on one input under an all-ones cotangent, run once per (device, case) and shared.
* ``BatchSession``: ``mst_logit_adam_init_batch`` / ``_step_batch`` on guarded buffers; ``online_ref.Session`` is the single-item
  session every item is compared with, bit for bit.
"""
import ctypes

import torch

import afprofile_ref as A
import online_ref as O
from oracle import loss_restated as ol

WEIGHTS = A.AF_WEIGHTS
MEAN_ULP = 2.0 ** -22  # two single fp32 roundings of float64 values formed from the same statistics: half an ulp each, of values <= max


# ================================================================ per-item feature loss ==========================================
def scrub(drv, extra=()):
    """Zero what a driver filled with NaN, before it is freed: torch's caching allocator hands freed blocks to the ``torch.empty`` of
    whatever runs next, and these tests are not about what other code does with NaN in memory it has not written."""
    for buf, _ in drv._all:
        buf.zero_()
    for buf in extra:
        buf.zero_()


class ItemsDriver(A.Driver):
    def workspace(self, nbytes):
        ws = super().workspace(nbytes)
        self.__dict__.setdefault("_workspaces", []).append(ws)
        return ws

    def scrub(self):
        scrub(self, self.__dict__.get("_workspaces", ()))

    def loss_items(self, pred, profile, weights, grad_losses=None):
        """pred (bs, 2, n) host tensor, profile (bs, 54) on the device, grad_losses (bs, 5) host tensor or None
        -> dict(losses (bs, 5), grad_pred (bs, 2, n)) on the host."""
        x = pred.float().contiguous().to(self.device)
        bs, _, n = x.shape
        nbytes = self.lib.mst_afloss_profile_workspace_bytes(bs, n)
        ws = self.workspace(nbytes)
        w = (ctypes.c_float * 5)(*weights)
        losses = self.guarded(bs * 5)
        prof = profile.contiguous()
        self.lib.mst_afloss_forward_profile_items(x, prof, bs, n, w, self.tables, self.fb, losses, ws, nbytes, self.stream_ptr())
        out = dict(losses=losses.view(bs, 5).cpu().clone())
        if grad_losses is not None:
            g = grad_losses.float().contiguous().to(self.device)
            assert tuple(g.shape) == (bs, 5)
            gx = self.guarded(x.numel())
            self.lib.mst_afloss_backward_profile_items(x, prof, bs, n, w, self.tables, self.fb, g, gx, ws, nbytes, self.stream_ptr())
            out["grad_pred"] = gx.view_as(x).cpu().clone()
        if x.is_cuda:  # the upload (on the host x may BE pred): the isolation case's NaN does not go back to the allocator
            x.zero_()
        return out


def audio(bs, n, m, seed=0):
    """Unit-scale noise with correlated channels: the prediction (bs, 2, n) and a target (bs, 2, m) of other statistics."""
    g = torch.Generator().manual_seed(7000 + 97 * bs + n + seed)
    x = torch.randn(bs, 2, n, generator=g)
    x[:, 1] = 0.6 * x[:, 1] + 0.3 * x[:, 0]
    y = 1.5 * torch.randn(bs, 2, m, generator=g) * torch.tensor([1.0, 0.5]).view(1, 2, 1)
    return x, y


_PAIRS = {}


def pair(drv, bs, n, m):
    """(x, profile, per-item result, batch result), both under an all-ones cotangent: computed once per device and case, never modified."""
    key = (drv.device.type, bs, n, m)
    if key not in _PAIRS:
        x, y = audio(bs, n, m)
        prof = drv.profile(y)
        items = drv.loss_items(x, prof, WEIGHTS, torch.ones(bs, 5))
        batch = drv.loss(x, prof, WEIGHTS, [1.0] * 5)
        drv.check_guards()
        for out in (items, batch):
            assert bool(torch.isfinite(out["losses"]).all()) and bool(torch.isfinite(out["grad_pred"]).all()), "an output element was not written"
        _PAIRS[key] = (x, prof, items, batch)
    return _PAIRS[key]


def check_batch_of_one(drv, n, m):
    """Check 1: bs = 1 is the batch call, bit for bit."""
    _, _, items, batch = pair(drv, 1, n, m)
    assert torch.equal(A.bits(items["losses"][0]), A.bits(batch["losses"]))
    assert torch.equal(A.bits(items["grad_pred"]), A.bits(batch["grad_pred"]))


def check_mean_over_items(drv, bs, n, m):
    """Check 2: the mean over the items is the batch call's value, to the two fp32 roundings."""
    _, _, items, batch = pair(drv, bs, n, m)
    rows = items["losses"].double()
    diff = (rows.mean(dim=0) - batch["losses"].double()).abs()
    bound = MEAN_ULP * rows.abs().max(dim=0).values
    print(f"\n[af items {bs}x2x{n}] |mean - batch| {diff.tolist()} bound {bound.tolist()}")
    assert bool((diff <= bound).all())


def check_scaling(drv, bs, n, m):
    """Check 3: for a power-of-two bs the per-item gradient under ones is exactly bs times the batch gradient under ones."""
    assert bs & (bs - 1) == 0
    _, _, items, batch = pair(drv, bs, n, m)
    assert torch.equal(items["grad_pred"], float(bs) * batch["grad_pred"])
    assert bool((items["grad_pred"] != 0).any())


def check_items_three_way(drv, bs, n, m, record=None):
    """Check 4: every item against the float64 oracle, with afprofile_ref's three-way bound (its factor, its floor)."""
    x, y = A.signals(bs, n, m)
    got = drv.loss_items(x, drv.profile(y), WEIGHTS, torch.tensor(A.COTANGENT).expand(bs, 5))
    drv.check_guards()
    triples = {}
    for b in range(bs):
        res = _item_reference(bs, n, m, b)
        A.assert_three_way(f"item {b} of {bs}x2x{n} vs {m}", got["losses"][b], got["grad_pred"][b:b + 1], res,
                           None if record is None else lambda b=b, **values: triples.update({f"item{b}_{k}": v for k, v in values.items()}))
    if record is not None:
        record(**triples)


_ITEM_REFS = {}


def _item_reference(bs, n, m, b):
    """{dtype: (five losses as float64, gradient)} of item b alone - a batch of one - by the oracle; computed once."""
    key = (bs, n, m, b)
    if key not in _ITEM_REFS:
        x, y = A.signals(bs, n, m)
        gw = torch.tensor(A.COTANGENT)
        res = {}
        for dt in (torch.float32, torch.float64):
            xo = x[b:b + 1].clone().to(dt).requires_grad_(True)
            lo = ol.audio_feature_loss(xo, y[b:b + 1].to(dt), WEIGHTS)
            vo = torch.stack([lo[k] for k in ol.AF_KEYS])
            (vo * gw.to(dt)).sum().backward()
            res[dt] = (vo.detach().double(), xo.grad)
        _ITEM_REFS[key] = res
    return _ITEM_REFS[key]


def check_isolation(drv, bs, n, m):
    """Check 5: a zero cotangent row gives an exactly zero gradient for that item alone; a NaN in one item's audio stays there."""
    assert bs == 3
    x, prof, base, _ = pair(drv, bs, n, m)
    g = torch.ones(bs, 5)
    g[1] = 0.0
    out = drv.loss_items(x, prof, WEIGHTS, g)
    assert bool((out["grad_pred"][1] == 0).all()), "a zero cotangent left a gradient"
    for b in (0, 2):
        assert torch.equal(A.bits(out["grad_pred"][b]), A.bits(base["grad_pred"][b]))
    assert torch.equal(A.bits(out["losses"]), A.bits(base["losses"]))
    bad = x.clone()
    bad[1, 0, n // 3] = float("nan")
    out = drv.loss_items(bad, prof, WEIGHTS, torch.ones(bs, 5))
    drv.check_guards()
    assert bool(torch.isnan(out["losses"][1]).any()), "the NaN did not reach its own item"
    for b in (0, 2):
        assert torch.equal(A.bits(out["losses"][b]), A.bits(base["losses"][b]))
        assert torch.equal(A.bits(out["grad_pred"][b]), A.bits(base["grad_pred"][b]))


def check_reproducible_and_refusals(drv, bs, n, m):
    """Check 6: a second call gives the same bits, guard regions stay intact, bad arguments launch nothing."""
    from mst import _cabi

    x, prof, base, _ = pair(drv, bs, n, m)
    again = drv.loss_items(x, prof, WEIGHTS, torch.ones(bs, 5))
    drv.check_guards()  # exactly bs * 5 losses and bs * 2 * n gradient elements between untouched guards
    assert torch.equal(A.bits(again["losses"]), A.bits(base["losses"])) and torch.equal(A.bits(again["grad_pred"]), A.bits(base["grad_pred"]))

    L, st = drv.lib, drv.stream_ptr()
    for name in ("mst_afloss_forward_profile_items", "mst_afloss_backward_profile_items"):
        assert hasattr(L, name) and name in _cabi.SIGNATURES
    xd = torch.zeros(bs, 2, n, device=drv.device)
    losses, gx = drv.guarded(bs * 5), drv.guarded(bs * 2 * n)
    g = torch.ones(bs, 5, device=drv.device)
    w = (ctypes.c_float * 5)(*WEIGHTS)
    nb = L.mst_afloss_profile_workspace_bytes(bs, n)  # the per-item calls take the batch calls' workspace
    ws = drv.workspace(nb)

    def refused(fn, *args):
        try:
            fn(*args)
        except _cabi.AbiError as e:
            assert e.code != 0
            return
        raise AssertionError(f"{fn.__name__} accepted {args}")

    good = dict(x=xd, bs=bs, n=n, tables=drv.tables, fb=drv.fb, prof=prof, ws=ws, w=w, losses=losses, g=g, gx=gx, nb=nb)
    for change in (dict(n=16384), dict(bs=0), dict(bs=-1), dict(x=None), dict(prof=None), dict(w=None), dict(tables=None), dict(fb=None),
                   dict(losses=None), dict(ws=None), dict(nb=nb - 4)):
        a = dict(good, **change)
        refused(L.mst_afloss_forward_profile_items, a["x"], a["prof"], a["bs"], a["n"], a["w"], a["tables"], a["fb"], a["losses"], a["ws"],
                a["nb"], st)
    for change in (dict(n=16384), dict(bs=0), dict(x=None), dict(prof=None), dict(w=None), dict(tables=None), dict(fb=None), dict(g=None),
                   dict(gx=None), dict(ws=None), dict(nb=nb - 4)):
        a = dict(good, **change)
        refused(L.mst_afloss_backward_profile_items, a["x"], a["prof"], a["bs"], a["n"], a["w"], a["tables"], a["fb"], a["g"], a["gx"],
                a["ws"], a["nb"], st)
    for t in (losses, gx, ws):
        assert bool(torch.isnan(t).all()), "a refused call wrote something"
    drv.check_guards()


# ================================================================ batched logit-Adam ============================================
class BatchSession:
    """``items`` optimiser states in one block; ``theta0[b]`` is item b's list of segments (host tensors, the same counts for every
    item).  Segment s lives in one guarded buffer of items * count elements, item-major, as a dense (items, ...) tensor does."""

    def __init__(self, drv, theta0, n_iters, n_terms):
        from mst import _cabi

        self.drv, self.cabi = drv, _cabi
        self.items = len(theta0)
        self.counts = [t.numel() for t in theta0[0]]
        self.n = sum(self.counts)
        self.theta = [drv.guarded(self.items * c) for c in self.counts]
        for s, dst in enumerate(self.theta):
            dst.copy_(torch.cat([theta0[b][s] for b in range(self.items)]))
        self.p = [drv.guarded(self.items * c) for c in self.counts]
        nbytes = drv.lib.mst_logit_adam_batch_state_bytes(self.items, self.n)
        assert nbytes == 4 * self.items * (O.HDR + 2 * self.n)
        self.state = drv.guarded(nbytes // 4).view(torch.int32).view(self.items, O.HDR + 2 * self.n)
        self.history = drv.guarded(n_iters * self.items * (1 + n_terms)).view(n_iters, self.items, 1 + n_terms)
        self.n_terms, self.calls = n_terms, 0
        drv.lib.mst_logit_adam_init_batch(self._segments([None] * len(self.counts)), len(self.counts), self.items, self.state,
                                          drv.stream_ptr())
        assert not bool(self.state.cpu().any()), "state not zeroed"

    def _segments(self, grads):
        seg = (self.cabi.LogitAdamSegment * len(self.counts))()
        for s, th, p, g, c in zip(seg, self.theta, self.p, grads, self.counts):
            s.theta, s.p, s.grad_p, s.count = th.data_ptr(), p.data_ptr(), None if g is None else g.data_ptr(), self.items * c
        return seg

    def step(self, grads, terms, lr, betas=O.BETAS, eps=O.EPS):
        """grads: per segment an (items, count) fp32 tensor on the driver's device or None; terms: (items, n_terms) there."""
        assert tuple(terms.shape) == (self.items, self.n_terms) and terms.is_contiguous()
        self.drv.lib.mst_logit_adam_step_batch(self._segments(grads), len(self.counts), self.items, terms, self.n_terms,
                                               self.history[self.calls], lr, betas[0], betas[1], eps, self.state, self.drv.stream_ptr())
        self.calls += 1

    def item(self, b):
        """(theta, p, first moments, second moments, header words 0..3, last history row) of item b, on the driver's device."""
        th = torch.cat([t.view(self.items, -1)[b] for t in self.theta])
        p = torch.cat([t.view(self.items, -1)[b] for t in self.p])
        st = self.state[b]
        return th, p, st[O.HDR:O.HDR + self.n], st[O.HDR + self.n:], st[:4], self.history[self.calls - 1, b]

    def words(self, b):
        return tuple(self.state[b, :4].cpu().tolist())


def _single_view(ses):
    """The same six of a single-item ``online_ref.Session``."""
    st = ses.state
    return (torch.cat(list(ses.theta)), torch.cat(list(ses.p)), st[O.HDR:O.HDR + ses.n], st[O.HDR + ses.n:O.HDR + 2 * ses.n], st[:4],
            ses.history[ses.calls - 1])


def _same(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def item_streams(counts, steps, scale, items, n_terms, seed=100):
    """Independent inputs per item: theta_0, a gradient stream per segment (steps, count), loss terms (steps, n_terms)."""
    theta0 = [O.start(counts, scale, seed + b) for b in range(items)]
    streams = [O.gradient_stream(counts, steps, seed + b)[0] for b in range(items)]
    g = torch.Generator().manual_seed(seed)
    terms = torch.rand(items, steps, n_terms, generator=g) + 0.5
    return theta0, streams, terms


def run_batch(drv, theta0, streams, terms, lr, null=(), per_step=None):
    """Every step of the items' streams through one BatchSession; per_step(k, session) after each step."""
    items, steps, n_terms = len(theta0), terms.shape[1], terms.shape[2]
    dev = drv.device
    ses = BatchSession(drv, theta0, steps, n_terms)
    up = [None if s in null else torch.stack([streams[b][s] for b in range(items)], dim=1).to(dev).contiguous()  # (steps, items, count)
          for s in range(len(ses.counts))]
    tm = terms.transpose(0, 1).to(dev).contiguous()  # (steps, items, n_terms)
    for k in range(steps):
        ses.step([None if u is None else u[k] for u in up], tm[k], lr)
        if per_step is not None:
            per_step(k, ses)
    return ses


def check_equal_to_independent_sessions(drv, items, counts, steps, lr, scale, n_terms=2):
    """Check 7: after every step, every item is bit for bit a single-item session fed the same stream."""
    theta0, streams, terms = item_streams(counts, steps, scale, items, n_terms)
    dev = drv.device
    singles = [O.Session(drv, theta0[b], steps, n_terms) for b in range(items)]
    ups = [[s.to(dev).contiguous() for s in streams[b]] for b in range(items)]
    tms = terms.to(dev).contiguous()

    def compare(k, ses):
        for b, one in enumerate(singles):
            one.step([s[k] for s in ups[b]], tms[b, k], lr)
            for name, x, y in zip(("theta", "p", "m", "v", "header", "history row"), ses.item(b), _single_view(one)):
                assert _same(x, y), f"item {b} of {items}, step {k}: {name} differs from the single-item session"

    ses = run_batch(drv, theta0, streams, terms, lr, per_step=compare)
    drv.check_guards()
    for b in range(items):
        assert ses.words(b) == (steps, 0, 0, steps)


def check_batch_nonfinite(drv, where, at=7, steps=20):
    """Check 8: a NaN in item 1's gradient or loss term at step 7 of 20 stops item 1 there and nowhere else."""
    counts, lr, items = O.STREAMS["song3"][0], 1e-3, 3
    theta0, streams, terms = item_streams(counts, steps, 1e-3, items, 2, seed=300)
    clean = run_batch(drv, theta0, streams, terms, lr)
    streams = [[s.clone() for s in item] for item in streams]
    terms = terms.clone()
    if where == "gradient":
        streams[1][2][at, 5] = float("nan")
    else:
        terms[1, at, 1] = float("nan")
    snaps = {}

    def snap(k, ses):
        if k in (at - 1, at, at + 1):
            snaps[k] = [t.clone() for t in ses.item(1)[:4]]

    ses = run_batch(drv, theta0, streams, terms, lr, per_step=snap)
    drv.check_guards()
    for a, b in zip(snaps[at], snaps[at - 1]):
        assert _same(a, b), "the rejected step changed something of item 1"
    assert not _same(snaps[at + 1][0], snaps[at][0]), "item 1 did not move in the step after it"
    assert ses.words(1) == (steps - 1, 1, at, steps)
    assert bool(torch.isfinite(ses.item(1)[0]).all())
    for b in (0, 2):
        assert ses.words(b) == (steps, 0, 0, steps)
        for name, x, y in zip(("theta", "p", "m", "v", "header"), ses.item(b), clean.item(b)):
            assert _same(x, y), f"item {b}: {name} differs from the run without the NaN"
        assert _same(ses.history[:, b], clean.history[:, b])
    h = ses.history[:, 1].cpu()
    assert torch.equal(O.bits(h[:, 1:]), O.bits(terms[1])), "a history row of item 1 was not written"


def check_batch_null_gradient(drv):
    """Check 9: a NULL-gradient segment keeps its bits for every item."""
    counts, lr, items, steps = O.STREAMS["song3"][0], 1e-3, 3, 10
    theta0, streams, terms = item_streams(counts, steps, 1e-3, items, 1, seed=500)
    first = BatchSession(drv, theta0, 1, 1)  # p as the init wrote it
    p0 = first.p[1].clone()
    ses = run_batch(drv, theta0, streams, terms, lr, null=(1,))
    drv.check_guards()
    assert _same(ses.theta[1], torch.cat([theta0[b][1] for b in range(items)]).to(drv.device)) and _same(ses.p[1], p0)
    lo, hi = counts[0], counts[0] + counts[1]
    for b in range(items):
        _, _, m, v, _, _ = ses.item(b)
        assert not bool(m[lo:hi].any()) and not bool(v[lo:hi].any())
        assert bool(m[:lo].any()) and bool(v[hi:].any())  # the other segments moved
        assert ses.words(b) == (steps, 0, 0, steps)


def check_batch_arguments(drv):
    """Check 10: items outside [1, 1024], a count that does not divide, and the single call's hyper-parameter cases launch nothing."""
    from mst import _cabi

    L, st = drv.lib, drv.stream_ptr()
    size = L.mst_logit_adam_batch_state_bytes
    assert size(0, 8) == 0 and size(1025, 8) == 0 and size(-1, 8) == 0 and size(2, 0) == 0 and size(2, (1 << 20) + 1) == 0
    assert size(1, 8) == L.mst_logit_adam_state_bytes(8) and size(3, 132) == 3 * 4 * (O.HDR + 2 * 132) and size(1024, 1 << 20) > 0
    items = 2
    theta, p, grad, row, term = (drv.guarded(8) for _ in range(5))
    state = drv.guarded(items * (O.HDR + 2 * 4))
    seg = (_cabi.LogitAdamSegment * 1)()
    seg[0].theta, seg[0].p, seg[0].grad_p, seg[0].count = theta.data_ptr(), p.data_ptr(), grad.data_ptr(), 8

    def refused(fn, *args):
        try:
            fn(*args)
        except _cabi.AbiError as e:
            assert e.code != 0
            return
        raise AssertionError(f"{fn.__name__} accepted {args}")

    good = dict(n_seg=1, items=items, terms=term, n_terms=1, row=row, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, state=state)
    for change in (dict(items=0), dict(items=1025), dict(items=-2), dict(items=3), dict(n_seg=0), dict(n_seg=5), dict(n_terms=0),
                   dict(n_terms=9), dict(terms=None), dict(row=None), dict(state=None), dict(lr=0.0), dict(lr=float("nan")), dict(b1=1.0),
                   dict(b2=-0.1), dict(eps=-1.0)):
        a = dict(good, **change)
        refused(L.mst_logit_adam_step_batch, seg, a["n_seg"], a["items"], a["terms"], a["n_terms"], a["row"], a["lr"], a["b1"], a["b2"],
                a["eps"], a["state"], st)
    for bad_items in (0, 1025, 3):  # 8 does not divide by 3
        refused(L.mst_logit_adam_init_batch, seg, 1, bad_items, state, st)
    refused(L.mst_logit_adam_init_batch, seg, 1, items, None, st)
    seg[0].p = None
    refused(L.mst_logit_adam_init_batch, seg, 1, items, state, st)
    for t in (theta, p, grad, row, term, state):
        assert bool(torch.isnan(t).all()), "a refused call wrote something"
    drv.check_guards()
