"""The shared cases of the best-iterate logit-Adam tests (tests/test_online_best_hostsim.py on the host simulator,
tests/test_online_best_gpu.py on the device).

TEST INFRASTRUCTURE.  Defined here once so that the two files cannot drift apart.  The driver, the guard regions, the gradient streams
and the single / batched sessions are those of tests/online_ref.py and tests/online_batch_ref.py, imported unchanged:

* ``BestSession`` / ``BatchBestSession``: ``mst_logit_adam_step_best`` / ``_step_best_batch`` on the sessions' guarded buffers plus a
  zero-filled ``best`` block between guards of its own.
* ``replay``: the rule of include/diffmst_hip.h in numpy fp32 - one fp32 subtraction, a strict ``<`` - on a list of losses.
* The loss terms are inputs and the gradient streams do not depend on theta, so a scripted list of losses has exact expectations; the
  expectations of ``SEQUENCE`` below are worked by hand from the rule and ``replay`` is held against them too.
"""
import ctypes

import numpy as np
import torch

import online_batch_ref as R
import online_ref as O

BEST_HDR = 16   # int32 words in front of the best logits
MAX_TERMS = 8   # MST_OPT_MAX_TERMS: the best block leaves room for a row of 1 + 8
COUNTS = (81, 25, 26)
SEQUENCE = [4.0, 3.0, 3.0, 2.75, 2.5, 2.5, 2.4, 2.3, 9.0, 1.0]
LR = 1e-3


def best_words(n):
    return BEST_HDR + n + 1 + MAX_TERMS


def replay(losses, min_delta=0.0, patience=0, skip=()):
    """-> (best iteration or None, best loss or None, wait count, iteration at which it settled or None).  ``skip``: the iterations
    that were not finite (they leave everything alone); iterations after the one that settled are frozen."""
    best_at, best, wait, settled = None, None, 0, None
    delta = np.float32(min_delta)
    for n, loss in enumerate(np.asarray(losses, dtype=np.float32)):
        if settled is not None:
            break
        if n in skip:
            continue
        if best_at is None or loss < np.float32(best - delta):
            best_at, best, wait = n, loss, 0
        else:
            wait += 1
        if patience > 0 and wait >= patience:
            settled = n
    return best_at, None if best is None else float(best), wait, settled


def _zeroed_best(drv, words):
    block = drv.guarded(words).view(torch.int32)
    block.zero_()  # the caller's part of the contract: all zero is "no best yet"
    return block


class BestSession(O.Session):
    def __init__(self, drv, theta0, n_iters, n_terms):
        super().__init__(drv, theta0, n_iters, n_terms)
        nbytes = drv.lib.mst_logit_adam_best_bytes(1, self.n)
        assert nbytes == 4 * best_words(self.n)
        self.best = _zeroed_best(drv, nbytes // 4)

    def step(self, grads, terms, lr, min_delta=0.0, patience=0, betas=O.BETAS, eps=O.EPS):
        assert terms.numel() == self.n_terms
        ptrs = (ctypes.c_void_p * self.n_terms)(*[terms.data_ptr() + 4 * j for j in range(self.n_terms)])
        self.drv.lib.mst_logit_adam_step_best(self._segments(grads), len(self.counts), ptrs, self.n_terms, self.history[self.calls], lr,
                                              betas[0], betas[1], eps, min_delta, patience, self.state, self.best, self.drv.stream_ptr())
        self.calls += 1

    def header(self):
        """(best iteration + 1, best loss, wait, settled + 1) with the loss as a float; the reserved words must be zero."""
        words = self.best[:BEST_HDR].cpu()
        assert not bool(words[4:].any()), "a reserved word of the best block was written"
        return int(words[0]), float(words[1:2].view(torch.float32)), int(words[2]), int(words[3])

    def best_logits(self):
        return self.best[BEST_HDR:BEST_HDR + self.n].cpu().view(torch.float32)

    def best_row(self):
        return self.best[BEST_HDR + self.n:BEST_HDR + self.n + 1 + self.n_terms].cpu().view(torch.float32)

    def everything(self):
        """theta, p, state words and moments, the best block: what a call may change besides its history row (host clones)."""
        return (torch.cat(self.thetas()), torch.cat([p.cpu() for p in self.p]), self.state.cpu().clone(), self.best.cpu().clone())


def scripted(drv, losses, min_delta, patience, counts=COUNTS, seed=11, nan_gradient_at=None, null=()):
    """A session fed ``losses`` as its one term and a seeded gradient stream -> (session, [everything() before each call] + [after the
    last])."""
    steps = len(losses)
    stream, _, _ = O.gradient_stream(counts, steps, seed)
    stream = [None if s in null else g.clone() for s, g in enumerate(stream)]
    if nan_gradient_at is not None:
        stream[2][nan_gradient_at, 7] = float("nan")
    ses = BestSession(drv, O.start(counts, 1e-3, seed), steps, 1)
    dev = drv.device
    up = [None if g is None else g.to(dev).contiguous() for g in stream]
    terms = torch.tensor(losses, dtype=torch.float32).view(steps, 1).to(dev)
    snaps = [ses.everything()]
    for k in range(steps):
        ses.step([None if g is None else g[k] for g in up], terms[k], LR, min_delta, patience)
        snaps.append(ses.everything())
    drv.check_guards()
    return ses, snaps


def same(a, b):
    return a.shape == b.shape and torch.equal(O.bits(a), O.bits(b))


def assert_frozen_call(snaps, k):
    """Call k changed nothing but its history row and the call count."""
    before, after = snaps[k], snaps[k + 1]
    assert same(before[0], after[0]) and same(before[1], after[1]) and same(before[3], after[3]), f"call {k} moved a frozen item"
    assert before[2][3] + 1 == after[2][3]
    changed = before[2] != after[2]
    changed[3] = False
    assert not bool(changed.any()), f"call {k} changed the state of a frozen item"


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def check_does_not_perturb(drv, name):
    """Case 1: with patience = 0 theta, p, the moments, the state words and every history row are the plain step's, bit for bit."""
    theta0, stream, _, _, _, lr = O.references(name)
    steps = stream[0].shape[0]
    terms = torch.rand(steps, 2, generator=torch.Generator().manual_seed(21)) + 0.5
    plain = O.Session(drv, theta0, steps, 2)
    plain.run(stream, lr, terms)
    ses = BestSession(drv, theta0, steps, 2)
    dev = drv.device
    up, tm = [s.to(dev).contiguous() for s in stream], terms.to(dev).contiguous()
    for k in range(steps):
        ses.step([s[k] for s in up], tm[k], lr, 0.0, 0)
    drv.check_guards()
    for name_, a, b in zip(("theta", "p"), (ses.theta, ses.p), (plain.theta, plain.p)):
        for x, y in zip(a, b):
            assert same(x, y), f"{name_} differs from mst_logit_adam_step"
    assert torch.equal(ses.state.cpu(), plain.state.cpu()), "state words or moments differ from mst_logit_adam_step"
    assert ses.words() == (steps, 0, 0, steps)
    assert same(ses.history, plain.history)
    total = terms[:, 0] + terms[:, 1]
    at, loss, wait, settled = replay(total.tolist())
    assert ses.header() == (at + 1, loss, wait, 0) and settled is None
    assert same(ses.best_row(), ses.history[at].cpu())


def check_scripted_sequence(drv):
    """Case 2: the hand-worked sequence, with and without a plateau rule."""
    ses, snaps = scripted(drv, SEQUENCE, 0.25, 3)
    assert replay(SEQUENCE, 0.25, 3) == (4, 2.5, 3, 7)  # the restatement agrees with the hand-worked figures
    assert ses.header() == (4 + 1, 2.5, 3, 7 + 1)
    assert ses.words() == (8, 0, 0, 10)
    for k in (8, 9):
        assert_frozen_call(snaps, k)
    assert not same(snaps[7][0], snaps[8][0]), "call 7, the one that settles the item, still updates it"
    assert same(ses.best_logits(), snaps[4][0]), "the stored logits are not theta as it was before call 4"
    assert same(ses.best_row(), ses.history[4].cpu()) and ses.best_row().tolist() == [2.5, 2.5]
    assert ses.history[:, 0].cpu().tolist() == torch.tensor(SEQUENCE).tolist()  # frozen calls write their rows

    ses, snaps = scripted(drv, SEQUENCE, 0.0, 0)
    assert replay(SEQUENCE) == (9, 1.0, 0, None)
    assert ses.header() == (9 + 1, 1.0, 0, 0)
    assert ses.words() == (10, 0, 0, 10)
    assert same(ses.best_logits(), snaps[9][0]) and same(ses.best_row(), ses.history[9].cpu())


def check_ties(drv):
    """Case 3: a tie keeps the earlier iterate."""
    ses, snaps = scripted(drv, [2.0, 1.0, 1.0, 3.0], 0.0, 0)
    assert ses.header() == (1 + 1, 1.0, 2, 0)
    assert same(ses.best_logits(), snaps[1][0]) and not same(snaps[1][0], snaps[2][0])


def check_nonfinite(drv, where):
    """Case 4: an Inf loss or a NaN gradient element at step 2 leaves the best block and its wait count alone; later iterations count
    on from there (3 does not improve on 3 - 0.25: wait 1; 4 is the best; 5, 6, 7 wait 1, 2, 3 and settle)."""
    losses = list(SEQUENCE)
    if where == "loss":
        losses[2] = float("inf")
    ses, snaps = scripted(drv, losses, 0.25, 3, nan_gradient_at=2 if where == "gradient" else None)
    for part in (0, 1, 3):
        assert same(snaps[2][part], snaps[3][part]), "the rejected call changed theta, p or the best block"
    assert tuple(snaps[3][3][:4].tolist()[i] for i in (0, 2, 3)) == (1 + 1, 0, 0)  # best at 1, wait 0, running
    assert tuple(snaps[3][2][:4].tolist()) == (2, 1, 2, 3)  # reported as the plain step reports it
    assert tuple(snaps[4][3][:4].tolist()[i] for i in (0, 2)) == (1 + 1, 1)  # iteration 3 counts on from the unchanged wait
    assert replay(losses, 0.25, 3, skip=(2,)) == (4, 2.5, 3, 7)
    assert ses.header() == (4 + 1, 2.5, 3, 7 + 1)
    assert ses.words() == (7, 1, 2, 10)
    assert same(ses.best_logits(), snaps[4][0])
    for k in (8, 9):
        assert_frozen_call(snaps, k)


def check_null_gradient(drv):
    """Case 5: a NULL-gradient segment is in the snapshot, with its start bits."""
    ses, snaps = scripted(drv, [3.0, 2.0, 1.0, 5.0], 0.0, 0, null=(1,))
    assert ses.header() == (2 + 1, 1.0, 1, 0)
    got, theta0 = ses.best_logits(), O.start(COUNTS, 1e-3, 11)
    assert same(got, snaps[2][0])
    assert same(got[81:106], theta0[1]) and not same(got[:81], theta0[0]) and not same(got[106:], theta0[2])


class BatchBestSession(R.BatchSession):
    def __init__(self, drv, theta0, n_iters, n_terms):
        super().__init__(drv, theta0, n_iters, n_terms)
        nbytes = drv.lib.mst_logit_adam_best_bytes(self.items, self.n)
        assert nbytes == 4 * self.items * best_words(self.n)
        self.best = _zeroed_best(drv, nbytes // 4).view(self.items, best_words(self.n))

    def step(self, grads, terms, lr, min_delta=0.0, patience=0, betas=O.BETAS, eps=O.EPS):
        assert tuple(terms.shape) == (self.items, self.n_terms) and terms.is_contiguous()
        self.drv.lib.mst_logit_adam_step_best_batch(self._segments(grads), len(self.counts), self.items, terms, self.n_terms,
                                                    self.history[self.calls], lr, betas[0], betas[1], eps, min_delta, patience,
                                                    self.state, self.best, self.drv.stream_ptr())
        self.calls += 1


def item_losses(items, steps, seed=31):
    """(items, steps) scripted losses on a grid of 0.25: item 0 always improves, item 1 never does after its first iteration, the rest
    are seeded draws."""
    g = torch.Generator().manual_seed(seed)
    losses = 0.25 * torch.randint(4, 40, (items, steps), generator=g).float()
    losses[0] = 100.0 - torch.arange(steps)
    if items > 1:
        losses[1] = 5.0
    return losses


def check_batch(drv, items, counts=COUNTS, steps=12, min_delta=0.25, patience=2):
    """Case 6: every item of a batch is bit for bit a single-item best session after every step; an item that settles freezes alone."""
    theta0, streams, _ = R.item_streams(counts, steps, 1e-3, items, 1, seed=700)
    losses = item_losses(items, steps)
    dev = drv.device
    singles = [BestSession(drv, theta0[b], steps, 1) for b in range(items)]
    ses = BatchBestSession(drv, theta0, steps, 1)
    ups = [[s.to(dev).contiguous() for s in streams[b]] for b in range(items)]
    stacked = [torch.stack([streams[b][s] for b in range(items)], dim=1).to(dev).contiguous() for s in range(len(counts))]
    tm = losses.to(dev).contiguous()  # (items, steps)
    for k in range(steps):
        ses.step([u[k] for u in stacked], tm[:, k:k + 1].contiguous(), LR, min_delta, patience)
        for b, one in enumerate(singles):
            one.step([s[k] for s in ups[b]], tm[b, k:k + 1], LR, min_delta, patience)
            mine = ses.item(b) + (ses.best[b],)
            alone = R._single_view(one) + (one.best,)
            for name, x, y in zip(("theta", "p", "m", "v", "header", "history row", "best block"), mine, alone):
                assert R._same(x, y), f"item {b} of {items}, step {k}: {name} differs from the single-item session"
    drv.check_guards()
    for b, one in enumerate(singles):
        at, loss, wait, settled = replay(losses[b].tolist(), min_delta, patience)
        assert one.header() == (at + 1, loss, wait, 0 if settled is None else settled + 1), f"item {b}"
        assert ses.words(b) == (steps if settled is None else settled + 1, 0, 0, steps)
    assert singles[0].header()[3] == 0 and ses.words(0)[0] == steps  # item 0 ran to the end ...
    if items > 1:
        assert singles[1].header() == (0 + 1, 5.0, 2, 2 + 1) and ses.words(1) == (3, 0, 0, steps)  # ... while item 1 froze after call 2


def check_lane_tails(drv, count):
    """Case 7: three items of one segment of ``count`` logits: the snapshot is complete, the guards on either side of ``best`` intact."""
    items, steps = 3, 3
    losses = torch.tensor([[3.0, 1.0, 2.0], [1.0, 2.0, 3.0], [3.0, 2.0, 1.0]])
    theta0, streams, _ = R.item_streams((count,), steps, 1e-3, items, 1, seed=900)
    dev = drv.device
    ses = BatchBestSession(drv, theta0, steps, 1)
    stacked = torch.stack([streams[b][0] for b in range(items)], dim=1).to(dev).contiguous()
    tm = losses.to(dev)
    before = []
    for k in range(steps):
        before.append(ses.theta[0].view(items, count).cpu().clone())
        ses.step([stacked[k]], tm[:, k:k + 1].contiguous(), LR)
    drv.check_guards()
    assert not same(before[0], before[1]) and not same(before[1], before[2])
    for b, at in enumerate((1, 0, 2)):
        block = ses.best[b].cpu()
        assert block[:4].tolist() == [at + 1, O.bits(torch.tensor(1.0)).item(), steps - 1 - at, 0] and not bool(block[4:BEST_HDR].any())
        assert same(block[BEST_HDR:BEST_HDR + count].view(torch.float32), before[at][b]), f"item {b}: the snapshot is not theta before call {at}"
        assert block[BEST_HDR + count:BEST_HDR + count + 2].view(torch.float32).tolist() == [1.0, 1.0]
        assert not bool(block[BEST_HDR + count + 2:].any()), "written past the history row"


def check_refusals(drv):
    """Case 8: the size function, and bad arguments that launch nothing."""
    from mst import _cabi

    L, st = drv.lib, drv.stream_ptr()
    for name in ("mst_logit_adam_best_bytes", "mst_logit_adam_step_best", "mst_logit_adam_step_best_batch"):
        assert hasattr(L, name) and name in _cabi.SIGNATURES
    size = L.mst_logit_adam_best_bytes
    assert size(1, 132) == 4 * (16 + 132 + 1 + 8) and size(3, 132) == 3 * 4 * (16 + 132 + 1 + 8) and size(1024, 1 << 20) > 0
    assert size(0, 8) == 0 and size(1025, 8) == 0 and size(-1, 8) == 0 and size(2, 0) == 0 and size(2, (1 << 20) + 1) == 0
    items = 2
    theta, p, grad, row, term = (drv.guarded(8) for _ in range(5))
    state, best = drv.guarded(items * (O.HDR + 2 * 4)), drv.guarded(items * best_words(4))
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

    good = dict(n_seg=1, items=items, terms=term, ptrs=ptrs, n_terms=1, row=row, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, delta=0.0,
                patience=0, state=state, best=best)
    new = (dict(best=None), dict(best=best.data_ptr() + 2), dict(delta=-1e-3), dict(delta=float("inf")), dict(delta=float("nan")),
           dict(delta=1e39), dict(patience=-1))
    old = (dict(n_seg=0), dict(n_seg=5), dict(n_terms=0), dict(n_terms=9), dict(row=None), dict(state=None), dict(lr=0.0),
           dict(lr=float("nan")), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0))
    for change in new + old + (dict(ptrs=None),):
        a = dict(good, **change)
        refused(L.mst_logit_adam_step_best, seg, a["n_seg"], a["ptrs"], a["n_terms"], a["row"], a["lr"], a["b1"], a["b2"], a["eps"],
                a["delta"], a["patience"], a["state"], a["best"], st)
    for change in new + old + (dict(terms=None), dict(items=0), dict(items=1025), dict(items=3)):
        a = dict(good, **change)
        refused(L.mst_logit_adam_step_best_batch, seg, a["n_seg"], a["items"], a["terms"], a["n_terms"], a["row"], a["lr"], a["b1"],
                a["b2"], a["eps"], a["delta"], a["patience"], a["state"], a["best"], st)
    for t in (theta, p, grad, row, term, state, best):
        assert bool(torch.isnan(t).all()), "a refused call wrote something"
    drv.check_guards()
