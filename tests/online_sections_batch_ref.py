"""The shared cases of the batched sectioned-fit tests: the step for ``items`` parameter sets with ``sections`` gradient rows each
(``mst_logit_adam_init_sections_batch`` / ``_step_sections_batch``) and ``AudioFeatureLoss.pooled(..., items=B)`` /
``profile(..., pool=True, items=B)``: tests/test_online_sections_batch_hostsim.py on the host simulator,
tests/test_online_sections_batch_gpu.py on the device.

TEST INFRASTRUCTURE.  Defined here once so that the two files cannot drift apart.  The drivers, guard regions, gradient streams, single
sessions and bounds are those of tests/online_ref.py, tests/online_batch_ref.py, tests/online_best_ref.py and
tests/online_sections_ref.py, imported unchanged:

* ``SectionsBatchSession``: the two new entry points on guarded buffers.  Every item of it is compared bit for bit with a session of an
  existing entry point: ``online_sections_ref.SectionSession`` fed that item's rows, ``online_ref.Session`` / ``online_best_ref.BestSession``
  fed the host's sequential fp32 sum of them (``host_sum``), ``online_batch_ref.BatchSession`` / ``online_best_ref.BatchBestSession`` at
  one section.
* ``SimLoss``: ``AudioFeatureLoss`` on the host simulator's library, for the loss-surface cases that run there.
"""
import torch

import afprofile_ref as A
import online_batch_ref as R
import online_best_ref as B
import online_ref as O
import online_sections_ref as P
from oracle import loss_restated as ol

COUNTS = O.STREAMS["song3"][0]  # (81, 25, 26)
STEPS = 50
WEIGHTS = A.AF_WEIGHTS


# ================================================================ the step ===========================================================
class SectionsBatchSession:
    """``items`` optimiser states over segments that start at ``theta0[b]`` (item b's list of host tensors); p has ``items * sections``
    rows per segment, item-major.  ``best``: with a zero-filled best block per item."""

    def __init__(self, drv, theta0, sections, n_iters, n_terms, best=False):
        from mst import _cabi

        self.drv, self.cabi, self.sections = drv, _cabi, sections
        self.items = len(theta0)
        self.counts = [t.numel() for t in theta0[0]]
        self.n = sum(self.counts)
        self.theta = [drv.guarded(self.items * c) for c in self.counts]
        for s, dst in enumerate(self.theta):
            dst.copy_(torch.cat([theta0[b][s] for b in range(self.items)]))
        self.p = [drv.guarded(self.items * sections * c) for c in self.counts]
        nbytes = drv.lib.mst_logit_adam_batch_state_bytes(self.items, self.n)
        self.state = drv.guarded(nbytes // 4).view(torch.int32).view(self.items, O.HDR + 2 * self.n)
        self.history = drv.guarded(n_iters * self.items * (1 + n_terms)).view(n_iters, self.items, 1 + n_terms)
        self.best = None
        if best:
            words = drv.lib.mst_logit_adam_best_bytes(self.items, self.n) // 4
            assert words == self.items * B.best_words(self.n)
            self.best = B._zeroed_best(drv, words).view(self.items, B.best_words(self.n))
        self.n_terms, self.calls = n_terms, 0
        drv.lib.mst_logit_adam_init_sections_batch(self._segments([None] * len(self.counts)), len(self.counts), self.items, sections,
                                                   self.state, drv.stream_ptr())
        assert not bool(self.state.cpu().any()), "state not zeroed"

    def _segments(self, grads):
        seg = (self.cabi.LogitAdamSegment * len(self.counts))()
        for s, th, p, g, c in zip(seg, self.theta, self.p, grads, self.counts):
            s.theta, s.p, s.grad_p, s.count = th.data_ptr(), p.data_ptr(), None if g is None else g.data_ptr(), self.items * c
        return seg

    def step(self, grads, terms, lr, min_delta=0.0, patience=0, betas=O.BETAS, eps=O.EPS):
        """grads: per segment an (items, sections, count) fp32 tensor on the driver's device or None; terms: (items, n_terms) there."""
        assert tuple(terms.shape) == (self.items, self.n_terms) and terms.is_contiguous()
        for g, c in zip(grads, self.counts):
            assert g is None or (tuple(g.shape) == (self.items, self.sections, c) and g.is_contiguous())
        self.drv.lib.mst_logit_adam_step_sections_batch(self._segments(grads), len(self.counts), self.items, self.sections, terms,
                                                        self.n_terms, self.history[self.calls], lr, betas[0], betas[1], eps, min_delta,
                                                        patience, self.state, self.best, self.drv.stream_ptr())
        self.calls += 1

    def rows(self, s, b):
        """Item b's (sections, count) rows of p of segment s."""
        return self.p[s].view(self.items, self.sections, self.counts[s])[b]

    def words(self, b):
        return tuple(self.state[b, :4].cpu().tolist())

    def everything(self, b):
        """What a call may change of item b besides its history row (host clones): theta, all rows of p, its state block, its best
        block."""
        th = torch.cat([t.view(self.items, -1)[b] for t in self.theta]).cpu().clone()
        p = torch.cat([self.rows(s, b).reshape(-1) for s in range(len(self.counts))]).cpu().clone()
        best = None if self.best is None else self.best[b].cpu().clone()
        return th, p, self.state[b].cpu().clone(), best


def assert_item_is_sections_session(ses, b, one, tag):
    """Item b against a single-item ``SectionSession`` (or, at one section, any single session whose p has one row): theta, every row
    of p, the whole state block, the history rows written so far, the best block."""
    for s, single in enumerate(one.theta):
        assert B.same(ses.theta[s].view(ses.items, -1)[b], single), f"{tag}: item {b}: theta of segment {s} differs"
    for s in range(len(ses.counts)):
        want = one.p[s].view(-1, ses.counts[s])
        want = want if want.shape[0] == ses.sections else want[:1].expand(ses.sections, -1)  # a one-row session: every row equals it
        assert B.same(ses.rows(s, b), want), f"{tag}: item {b}: a row of p of segment {s} differs"
    assert torch.equal(ses.state[b].cpu(), one.state.cpu()), f"{tag}: item {b}: state words or moments differ"
    assert B.same(ses.history[:ses.calls, b], one.history[:one.calls]), f"{tag}: item {b}: history differs"
    if ses.best is not None:
        assert torch.equal(ses.best[b].cpu(), one.best.cpu()), f"{tag}: item {b}: best block differs"


def item_section_streams(counts, steps, items, sections, seed=100):
    """-> streams[b][s]: a (steps, sections, count) host stream of gradients, independent per item and section."""
    return [P.section_streams(counts, steps, sections, seed=seed + 1000 * b) for b in range(items)]


def stacked(streams, dev):
    """streams[b][s] (steps, sections, count) -> per segment (steps, items, sections, count) on the device."""
    return [torch.stack([streams[b][s] for b in range(len(streams))], dim=1).to(dev).contiguous() for s in range(len(streams[0]))]


def item_terms(items, steps, n_terms, seed=45):
    return torch.rand(steps, items, n_terms, generator=torch.Generator().manual_seed(seed)) + 0.5


def check_one_item_is_the_sections_call(drv, counts, best, sections=3, steps=STEPS, scale=1e-3, lr=1e-3):
    """Check 1: items = 1 against mst_logit_adam_init_sections / _step_sections, plain and with a best block, bit for bit."""
    theta0 = O.start(counts, scale, 0)
    streams = P.section_streams(counts, steps, sections)
    terms = item_terms(1, steps, 2)
    dev = drv.device
    one = P.SectionSession(drv, theta0, sections, steps, 2, best=best)
    ses = SectionsBatchSession(drv, [theta0], sections, steps, 2, best=best)
    up, tm = [s.to(dev).contiguous() for s in streams], terms.to(dev).contiguous()
    extra = (0.01, 4) if best else ()
    for k in range(steps):
        one.step([s[k] for s in up], tm[k, 0], lr, *extra)
        ses.step([s[k:k + 1] for s in up], tm[k], lr, *extra)
        if k % 7 == 0 or k == steps - 1:  # a difference never heals: theta, the moments and the history carry it to the last step
            assert_item_is_sections_session(ses, 0, one, f"items = 1, {counts}, step {k}")
    drv.check_guards()
    if not best:
        assert ses.words(0) == (steps, 0, 0, steps)


def check_one_section_is_the_batch_call(drv, items, best, counts=COUNTS, steps=STEPS, lr=1e-3):
    """Check 2: sections = 1 against mst_logit_adam_init_batch / _step_batch / _step_best_batch, bit for bit."""
    theta0, streams, terms = R.item_streams(counts, steps, 1e-3, items, 2)
    dev = drv.device
    batch = (B.BatchBestSession if best else R.BatchSession)(drv, theta0, steps, 2)
    ses = SectionsBatchSession(drv, theta0, 1, steps, 2, best=best)
    up = [torch.stack([streams[b][s] for b in range(items)], dim=1).to(dev).contiguous() for s in range(len(counts))]  # (steps, items, count)
    tm = terms.transpose(0, 1).to(dev).contiguous()
    extra = (0.01, 4) if best else ()
    for k in range(steps):
        batch.step([u[k] for u in up], tm[k], lr, *extra)
        ses.step([u[k].unsqueeze(1) for u in up], tm[k], lr, *extra)
        if k % 7 == 0 or k == steps - 1:
            for a, b_ in zip(ses.theta + ses.p, batch.theta + batch.p):
                assert B.same(a, b_), f"sections = 1, step {k}: theta or p differs from the batch call"
            assert torch.equal(ses.state.cpu(), batch.state.cpu()), f"sections = 1, step {k}: state differs from the batch call"
            assert B.same(ses.history[:k + 1], batch.history[:k + 1])
            if best:
                assert torch.equal(ses.best.cpu(), batch.best.cpu()), f"sections = 1, step {k}: best block differs from the batch call"
    drv.check_guards()


def check_items_of_sections(drv, items, sections, counts=COUNTS, steps=STEPS, lr=1e-3, scale=1e-3, best=False, with_sum=True):
    """Check 3: every item bit for bit an independent single-item _step_sections session fed that item's rows and - ``with_sum`` - a
    single mst_logit_adam_step (_step_best) session fed the host's sequential fp32 sum of them (the two say the same: the sections
    session is pinned to the summed single session by tests/online_sections_ref.py)."""
    theta0 = [O.start(counts, scale, 20 + b) for b in range(items)]
    streams = item_section_streams(counts, steps, items, sections)
    terms = item_terms(items, steps, 2)
    dev = drv.device
    alone = [P.SectionSession(drv, theta0[b], sections, steps, 2, best=best) for b in range(items)]
    summed = [(B.BestSession if best else O.Session)(drv, theta0[b], steps, 2) for b in range(items)] if with_sum else []
    ses = SectionsBatchSession(drv, theta0, sections, steps, 2, best=best)
    up, tm = stacked(streams, dev), terms.to(dev).contiguous()
    sums = [[torch.stack([P.host_sum(s[k]) for k in range(steps)]).to(dev) for s in streams[b]] for b in range(len(summed))]
    extra = (0.01, 4) if best else ()
    for k in range(steps):
        ses.step([u[k] for u in up], tm[k], lr, *extra)
        for b in range(items):
            alone[b].step([u[k, b] for u in up], tm[k, b], lr, *extra)
        for b, one in enumerate(summed):
            one.step([s[k] for s in sums[b]], tm[k, b], lr, *extra)
        if k % 7 == 0 or k == steps - 1:
            for b in range(items):
                assert_item_is_sections_session(ses, b, alone[b], f"{items} x {sections} of {counts}, step {k}")
            for b, one in enumerate(summed):
                assert_item_is_sections_session(ses, b, one, f"{items} x {sections} of {counts} vs host_sum, step {k}")
    drv.check_guards()
    if not best:
        for b in range(items):
            assert ses.words(b) == (steps, 0, 0, steps)


def check_nonfinite_item(drv, where, at=3, steps=6, items=3, sections=3):
    """Check 4: a NaN addend, or two finite addends whose sum overflows, in item 1 of 3 at step 3 of 6: item 1's iteration changes
    nothing and is the one reported; items 0 and 2 are bit for bit a run without the fault."""
    counts, lr = COUNTS, 1e-3
    theta0 = [O.start(counts, 1e-3, 30 + b) for b in range(items)]
    streams = item_section_streams(counts, steps, items, sections, seed=200)
    terms = item_terms(items, steps, 2, seed=46)
    dev = drv.device

    def run(streams):
        ses = SectionsBatchSession(drv, theta0, sections, steps, 2)
        up, tm = stacked(streams, dev), terms.to(dev).contiguous()
        snaps = []
        for k in range(steps):
            ses.step([u[k] for u in up], tm[k], lr)
            snaps.append([ses.everything(b) for b in range(items)])
        return ses, snaps

    clean, clean_snaps = run(streams)
    faulty = [[s.clone() for s in item] for item in streams]
    if where == "nan":
        faulty[1][2][at, 1, 7] = float("nan")
    else:
        faulty[1][0][at, 0, 5] = 3e38
        faulty[1][0][at, 1, 5] = 3e38
        assert bool(torch.isfinite(faulty[1][0][at]).all()) and not bool(torch.isfinite(P.host_sum(faulty[1][0][at])).all())
    ses, snaps = run(faulty)
    drv.check_guards()
    for part in (0, 1):  # theta, p; and the moments
        assert B.same(snaps[at][1][part], snaps[at - 1][1][part]), "the rejected step changed theta or p of item 1"
    assert torch.equal(snaps[at][1][2][O.HDR:], snaps[at - 1][1][2][O.HDR:]), "the rejected step changed the moments of item 1"
    assert not B.same(snaps[at + 1][1][0], snaps[at][1][0]), "item 1 did not move in the step after it"
    assert bool(torch.isfinite(snaps[-1][1][0]).all())
    assert ses.words(1) == (steps - 1, 1, at, steps)
    for b in (0, 2):
        assert ses.words(b) == (steps, 0, 0, steps)
        for k in range(steps):
            for x, y in zip(snaps[k][b][:3], clean_snaps[k][b][:3]):
                assert torch.equal(O.bits(x), O.bits(y)), f"item {b}, step {k}: differs from the run without the fault"
        assert B.same(ses.history[:, b], clean.history[:, b])
    h = ses.history[:, 1].cpu()
    assert torch.equal(O.bits(h[:, 1:]), O.bits(terms[:, 1])), "a history row of item 1 was not written"


def check_null_gradient(drv, items=3, sections=3, steps=10):
    """Check 6: a NULL-gradient segment keeps theta, the moments and all rows of p for every item."""
    counts, lr = COUNTS, 1e-3
    theta0 = [O.start(counts, 1e-3, 40 + b) for b in range(items)]
    streams = item_section_streams(counts, steps, items, sections, seed=300)
    dev = drv.device
    ses = SectionsBatchSession(drv, theta0, sections, steps, 1)
    p0 = ses.p[1].clone()
    up, term = stacked(streams, dev), torch.ones(items, 1, device=dev)
    for k in range(steps):
        ses.step([None if s == 1 else u[k] for s, u in enumerate(up)], term, lr)
    drv.check_guards()
    assert B.same(ses.theta[1], torch.cat([theta0[b][1] for b in range(items)]).to(dev)) and B.same(ses.p[1], p0)
    lo, hi = counts[0], counts[0] + counts[1]
    for b in range(items):
        for r in range(sections):
            assert B.same(ses.rows(1, b)[r], ses.rows(1, b)[0]) and B.same(ses.rows(0, b)[r], ses.rows(0, b)[0])
        st = ses.state[b].cpu()
        m, v = st[O.HDR:O.HDR + ses.n], st[O.HDR + ses.n:]
        assert not bool(m[lo:hi].any()) and not bool(v[lo:hi].any()) and bool(m[:lo].any()) and bool(v[hi:].any())
        assert ses.words(b) == (steps, 0, 0, steps)


def item_sequences():
    """Three scripted loss sequences, one per item: online_best_ref's hand-worked one, a constant and an ever-improving one."""
    steps = len(B.SEQUENCE)
    return [list(B.SEQUENCE), [5.0] * steps, [100.0 - k for k in range(steps)]]


def check_scripted_sequences(drv, sections=3, min_delta=0.25, patience=2):
    """Check 7: DESIGN 22's scripted sequence per item, a different one for every item: the single best kernel's verdicts and bits on
    the summed gradients; a settled item is frozen while the others go on."""
    counts, losses = B.COUNTS, item_sequences()
    items, steps = len(losses), len(B.SEQUENCE)
    theta0 = [O.start(counts, 1e-3, 50 + b) for b in range(items)]
    streams = item_section_streams(counts, steps, items, sections, seed=400)
    dev = drv.device
    singles = [B.BestSession(drv, theta0[b], steps, 1) for b in range(items)]
    ses = SectionsBatchSession(drv, theta0, sections, steps, 1, best=True)
    up = stacked(streams, dev)
    sums = [[torch.stack([P.host_sum(s[k]) for k in range(steps)]).to(dev) for s in streams[b]] for b in range(items)]
    tm = torch.tensor(losses, dtype=torch.float32).t().contiguous().view(steps, items, 1).to(dev)
    snaps = [[ses.everything(b) for b in range(items)]]
    for k in range(steps):
        ses.step([u[k] for u in up], tm[k], B.LR, min_delta, patience)
        for b, one in enumerate(singles):
            one.step([s[k] for s in sums[b]], tm[k, b], B.LR, min_delta, patience)
            assert_item_is_sections_session(ses, b, one, f"scripted, step {k}")
        snaps.append([ses.everything(b) for b in range(items)])
    drv.check_guards()
    # worked by hand from the rule of include/diffmst_hip.h: 4; 3 improves; 3 and 2.75 (not below 3 - 0.25) wait 1, 2: settled at 3
    assert B.replay(losses[0], min_delta, patience) == (1, 3.0, 2, 3) and singles[0].header() == (1 + 1, 3.0, 2, 3 + 1)
    assert B.replay(losses[1], min_delta, patience) == (0, 5.0, 2, 2) and singles[1].header() == (0 + 1, 5.0, 2, 2 + 1)
    assert B.replay(losses[2], min_delta, patience) == (steps - 1, 100.0 - (steps - 1), 0, None) and singles[2].header()[3] == 0
    assert ses.words(0) == (4, 0, 0, steps) and ses.words(1) == (3, 0, 0, steps) and ses.words(2) == (steps, 0, 0, steps)
    for b, settled in ((0, 3), (1, 2)):  # frozen from the call after the one that settled it: its row and call count, nothing else
        for k in range(settled + 1, steps):
            before, after = snaps[k][b], snaps[k + 1][b]
            assert B.same(before[0], after[0]) and B.same(before[1], after[1]) and torch.equal(before[3], after[3]), f"call {k} moved item {b}"
            changed = before[2] != after[2]
            changed[3] = False
            assert before[2][3] + 1 == after[2][3] and not bool(changed.any()), f"call {k} changed the state of frozen item {b}"
        assert not B.same(snaps[settled][b][0], snaps[settled + 1][b][0]), "the call that settles an item still updates it"
    for k in range(steps):  # ... while item 2 goes on
        assert not B.same(snaps[k][2][0], snaps[k + 1][2][0])
    assert ses.history[:, :, 0].cpu().tolist() == torch.tensor(losses).t().tolist()  # frozen calls write their rows


def check_refusals(drv):
    """Check 8: items 0 and 1025, sections 0 and 65, a count that items does not divide, misaligned and NULL pointers and the
    hyper-parameter cases of the batch and sections calls launch nothing and write nothing."""
    from mst import _cabi

    L, st = drv.lib, drv.stream_ptr()
    for name in ("mst_logit_adam_init_sections_batch", "mst_logit_adam_step_sections_batch"):
        assert hasattr(L, name) and name in _cabi.SIGNATURES
    assert L.mst_abi_version() == _cabi.ABI_VERSION == 13
    items, sections, c = 2, 2, 4
    theta, row, term = drv.guarded(items * c), drv.guarded(items * 2), drv.guarded(items)
    p, grad = drv.guarded(items * sections * c), drv.guarded(items * sections * c)
    state, best = drv.guarded(items * (O.HDR + 2 * c)), drv.guarded(items * B.best_words(c))
    seg = (_cabi.LogitAdamSegment * 1)()

    def fill(theta_ptr=theta.data_ptr(), p_ptr=p.data_ptr(), grad_ptr=grad.data_ptr(), count=items * c):
        seg[0].theta, seg[0].p, seg[0].grad_p, seg[0].count = theta_ptr, p_ptr, grad_ptr, count

    def refused(fn, *args):
        try:
            fn(*args)
        except _cabi.AbiError as e:
            assert e.code != 0
            return
        raise AssertionError(f"{fn.__name__} accepted {args}")

    good = dict(seg=seg, n_seg=1, items=items, S=sections, terms=term, n_terms=1, row=row, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, delta=0.0,
                patience=0, state=state, best=None)

    def step(**change):
        a = dict(good, **change)
        refused(L.mst_logit_adam_step_sections_batch, a["seg"], a["n_seg"], a["items"], a["S"], a["terms"], a["n_terms"], a["row"],
                a["lr"], a["b1"], a["b2"], a["eps"], a["delta"], a["patience"], a["state"], a["best"], st)

    def init(**change):
        a = dict(good, **change)
        refused(L.mst_logit_adam_init_sections_batch, a["seg"], a["n_seg"], a["items"], a["S"], a["state"], st)

    fill()
    for change in (dict(items=0), dict(items=1025), dict(items=-2), dict(items=3), dict(S=0), dict(S=65), dict(S=-1), dict(seg=None),
                   dict(n_seg=0), dict(n_seg=5), dict(state=None), dict(state=state.data_ptr() + 2)):
        init(**change)
        step(**change)
    for change in (dict(terms=None), dict(terms=term.data_ptr() + 2), dict(n_terms=0), dict(n_terms=9), dict(row=None),
                   dict(row=row.data_ptr() + 2), dict(lr=0.0), dict(lr=float("nan")), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0),
                   dict(best=best, delta=-1e-3), dict(best=best, delta=float("nan")), dict(best=best, delta=1e39),
                   dict(best=best, patience=-1), dict(best=best.data_ptr() + 2)):
        step(**change)
    for bad in (dict(theta_ptr=None), dict(p_ptr=None), dict(theta_ptr=theta.data_ptr() + 2), dict(p_ptr=p.data_ptr() + 2),
                dict(grad_ptr=grad.data_ptr() + 2), dict(count=0), dict(count=items * c + 1)):
        fill(**bad)
        init()
        step()
    for t in (theta, p, grad, row, term, state, best):
        assert bool(torch.isnan(t).all()), "a refused call wrote something"
    drv.check_guards()


# ================================================================ the loss surface ====================================================
class SimLoss:
    """``AudioFeatureLoss.pooled`` / ``.profile`` with ``mst._hip`` pointed at a host library (the simulator's): the Python surface on
    host tensors.  A context manager; everything is put back on exit."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        import contextlib

        from mst import _hip, loss

        self._saved = (_hip.lib, _hip.require_cuda, _hip.launch_on, loss._af_constants)
        tables = torch.zeros(self.lib.mst_afloss_tables_bytes() // 4)
        self.lib.mst_afloss_init_tables(tables, None)
        fbs = {}

        def constants(dev, sample_rate):
            from mst.filter import barkscale_fbanks

            if sample_rate not in fbs:
                fbs[sample_rate] = barkscale_fbanks(16385, 20.0, 20000.0, 24, sample_rate).contiguous()
            return tables, fbs[sample_rate]

        @contextlib.contextmanager
        def launch_on(dev):
            yield None

        _hip.lib, _hip.require_cuda, _hip.launch_on, loss._af_constants = (lambda: self.lib), (lambda *a: None), launch_on, constants
        return loss.AudioFeatureLoss(WEIGHTS, 44100)

    def __exit__(self, *exc):
        from mst import _hip, loss

        _hip.lib, _hip.require_cuda, _hip.launch_on, loss._af_constants = self._saved
        return False


def peak_scaled_audio(items, sections, n, m, seed=0):
    """``online_sections_ref.sections_audio`` with the section scales rotated by the item index: the pooled peak of item b sits in
    section (sections - 1 - b) mod sections - a different section per item.  -> x (items * sections, 2, n), y (items, 2, m)."""
    x, y = P.sections_audio(items, sections, n, m, seed)
    base = 0.5 * (1.0 + torch.arange(sections, dtype=torch.float32))
    x = x / base.repeat(items).view(-1, 1, 1)
    scale = torch.cat([base.roll(-b) for b in range(items)])
    return x * scale.view(-1, 1, 1), y


_REFS = {}


def references(items, sections, n, m):
    """(x, y, [per item {dtype: (five losses as float64, gradient (S, 2, n))}]) by ``online_sections_ref.pooled_loss``: computed once,
    shared, never modified; the premise of the three-way bound is checked as ``online_sections_ref.references`` checks it."""
    key = (items, sections, n, m)
    if key not in _REFS:
        x, y = peak_scaled_audio(items, sections, n, m)
        gw = torch.tensor(A.COTANGENT)
        res, where = [], []
        for item in range(items):
            xs, per = x[item * sections:(item + 1) * sections], {}
            peaks = xs.abs().amax(dim=-1).double()
            for ch in range(2):
                q = peaks[:, ch].sort().values
                assert bool(((q[1:] - q[:-1]) / q[1:] > 1e-3).all()), "two section peaks too close"
            where.append(int(peaks[:, 0].argmax()))
            whole = torch.cat(list(xs), dim=-1)
            assert float(whole.pow(2).mean(dim=-1).min()) > 1e-6 and float((whole[0] + whole[1]).pow(2).mean()) > 1e-6
            for dt in (torch.float32, torch.float64):
                xo = xs.clone().to(dt).requires_grad_(True)
                vo = P.pooled_loss(xo, y[item:item + 1], WEIGHTS)
                (vo * gw.to(dt)).sum().backward()
                assert bool(torch.isfinite(vo).all()) and bool(torch.isfinite(xo.grad).all())
                per[dt] = (vo.detach().double(), xo.grad)
            res.append(per)
        assert len(set(where)) == min(items, sections), f"the pooled peaks sit in sections {where}"  # a different section per item
        _REFS[key] = (x, y, res)
    return _REFS[key]


def pooled_call(loss, x, target, items, cotangent=None):
    """``loss.pooled(x, target, items=items)`` and its gradient under ``cotangent`` (items, 5) (default: afprofile_ref.COTANGENT for
    every item) -> (losses (items, 5), gradient like x), on the host."""
    leaf = x.clone().requires_grad_(True)
    out = loss.pooled(leaf, target, items=items)
    assert list(out) == list(ol.AF_KEYS)
    terms = list(out.values())
    for t in terms:
        assert tuple(t.shape) == (items,) and t.dtype == torch.float32
    g = torch.tensor(A.COTANGENT).expand(items, 5) if cotangent is None else cotangent
    g = g.to(x.device)
    grad, = torch.autograd.grad(terms, leaf, [g[:, k].contiguous() for k in range(5)])
    return torch.stack([t.detach() for t in terms], dim=1).cpu(), grad.cpu()


def check_items_one_is_todays_call(loss, dev, n, m, thorough=True):
    """Check L1: pooled(x, target, items=1) and profile(x, pool=True, items=1) are the calls without ``items``, bit for bit.  Without
    ``thorough`` (the simulator, seconds per row): the five terms only; the gradient and the profile are device cases."""
    x, y = P.sections_audio(1, 2, n, m)
    x, y = x.to(dev), y.to(dev)
    if thorough:
        a, b = loss.profile(x, pool=True), loss.profile(x, pool=True, items=1)
        assert a.batch_size == b.batch_size == 1 and a.n_samples == b.n_samples == 2 * n and torch.equal(A.bits(a.data), A.bits(b.data))
    target = loss.profile(y)
    la, lb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    oa, ob = loss.pooled(la, target), loss.pooled(lb, target, items=1)
    assert list(oa) == list(ob)
    for k in oa:
        assert tuple(oa[k].shape) == tuple(ob[k].shape) == (1,) and torch.equal(A.bits(oa[k]), A.bits(ob[k]))
        assert oa[k].requires_grad and ob[k].requires_grad
    if thorough:
        g = torch.tensor(A.COTANGENT, device=dev)
        ga, = torch.autograd.grad(list(oa.values()), la, [g[k:k + 1] for k in range(5)])
        gb, = torch.autograd.grad(list(ob.values()), lb, [g[k:k + 1] for k in range(5)])
        assert torch.equal(A.bits(ga), A.bits(gb)) and bool((ga != 0).any())


_BASE = {}


def base_call(loss, dev, items, sections, n, m):
    """(x, y, the profile of y, losses, gradient) of the case of ``references`` under afprofile_ref.COTANGENT: run once per device
    and case, shared by the cases below, never modified."""
    key = (torch.device(dev).type, items, sections, n, m)
    if key not in _BASE:
        x, y, _ = references(items, sections, n, m)
        xd, yd = x.to(dev), y.to(dev)
        target = loss.profile(yd)
        assert target.batch_size == items
        _BASE[key] = (xd, yd, target) + pooled_call(loss, xd, target, items)
    return _BASE[key]


def check_pooled_three_way(loss, dev, items, sections, n, m, record=None, second_run=True):
    """Check L2: every item against the float64 restatement, afprofile_ref's three-way bound; ``second_run``: a second run, its
    target the (items, 2, m) tensor itself (profiled on the way), gives the same bits."""
    _, _, res = references(items, sections, n, m)
    xd, yd, _, losses, grad = base_call(loss, dev, items, sections, n, m)
    triples = {}
    for item in range(items):
        rows = slice(item * sections, (item + 1) * sections)
        A.assert_three_way(f"pooled(items={items}) item {item} of {items}x{sections}x2x{n} vs {m}", losses[item], grad[rows], res[item],
                           None if record is None else lambda item=item, **values: triples.update({f"item{item}_{k}": v for k, v in values.items()}))
    if record is not None:
        record(**triples)
    if second_run:
        l2, g2 = pooled_call(loss, xd, yd, items)
        assert torch.equal(A.bits(l2), A.bits(losses)) and torch.equal(A.bits(g2), A.bits(grad))


def check_isolation(loss, dev, items, sections, n, m, separately=True):
    """Check L3: changing item 1's audio, profile row or cotangent, one at a time, leaves item 0's losses and gradient rows
    bit-identical; a cotangent on element b reaches item b's rows only.  Without ``separately`` (the simulator, seconds per row) ONE
    call says it: item 1's audio and profile row changed and its cotangent zero - item 0 keeps its bits, item 1's losses move, and
    item 1's gradient rows are exactly zero."""
    xd, _, target, base_l, base_g = base_call(loss, dev, items, sections, n, m)
    mine, theirs = slice(0, sections), slice(sections, 2 * sections)
    audio = xd.clone()
    audio[theirs] = audio[theirs].flip(-1) * 0.5
    data = target.data.clone()
    data[1] = data[1] * 1.5
    profile = type(target)(data, target.sample_rate)
    cot = torch.tensor(A.COTANGENT).expand(items, 5).clone()
    if not separately:
        cot[1] = 0.0
        l, g = pooled_call(loss, audio, profile, items, cot)
        assert torch.equal(A.bits(l[0]), A.bits(base_l[0])) and torch.equal(A.bits(g[mine]), A.bits(base_g[mine])), "item 1 reached item 0"
        assert not torch.equal(A.bits(l[1]), A.bits(base_l[1])), "the change did not reach item 1 itself"
        assert bool((g[theirs] == 0).all()), "a cotangent on element 0 reached item 1's rows"
        return
    cot[1] = cot[1] * -3.0
    for x_, target_, cot_ in [(audio, target, None), (xd, profile, None), (xd, target, cot)]:
        l, g = pooled_call(loss, x_, target_, items, cot_)
        assert torch.equal(A.bits(l[0]), A.bits(base_l[0])) and torch.equal(A.bits(g[mine]), A.bits(base_g[mine])), "item 1 reached item 0"
        assert not torch.equal(A.bits(g[theirs]), A.bits(base_g[theirs])), "the change did not reach item 1 itself"
        if cot_ is None:
            assert not torch.equal(A.bits(l[1]), A.bits(base_l[1]))
        else:
            assert torch.equal(A.bits(l), A.bits(base_l))  # a cotangent changes no loss
    for b in range(items):
        cot = torch.zeros(items, 5)
        cot[b] = torch.tensor(A.COTANGENT)
        _, g = pooled_call(loss, xd, target, items, cot)
        rows = torch.zeros(items * sections, dtype=torch.bool)
        rows[b * sections:(b + 1) * sections] = True
        assert bool((g[~rows] == 0).all()) and torch.equal(A.bits(g[rows]), A.bits(base_g[rows])), f"a cotangent on element {b}"


def check_broadcast_and_own_profile(loss, dev, items, sections, n, m):
    """Checks L4, L5: a profile of batch size 1 is that row repeated; the loss of the sections against their own
    profile(pool=True, items=B) is exactly 0 in all five terms for every item.  That profile is, row by row, every item's own
    pooled profile, and a second run of it gives the same bits.  (A device case: the simulator takes seconds per row.)"""
    xd, _, target = base_call(loss, dev, items, sections, n, m)[:3]
    one = type(target)(target.data[:1].clone(), target.sample_rate)
    assert one.batch_size == 1
    repeated = type(one)(one.data.repeat(items, 1), one.sample_rate)
    la, ga = pooled_call(loss, xd, one, items)
    lb, gb = pooled_call(loss, xd, repeated, items)
    assert torch.equal(A.bits(la), A.bits(lb)) and torch.equal(A.bits(ga), A.bits(gb))
    own = loss.profile(xd, pool=True, items=items)
    assert own.batch_size == items and own.n_samples == sections * n
    again = loss.profile(xd, pool=True, items=items)
    assert torch.equal(A.bits(own.data), A.bits(again.data))
    for b in range(items):  # item b's row is the pooled profile of its own rows
        alone = loss.profile(xd[b * sections:(b + 1) * sections], pool=True)
        assert torch.equal(A.bits(own.data[b:b + 1]), A.bits(alone.data))
    out = loss.pooled(xd, own, items=items)
    z = torch.stack(list(out.values()), dim=1).cpu()
    assert tuple(z.shape) == (items, 5) and bool((z == 0).all()), z.tolist()


def check_loss_refusals(loss, dev, n=17000):
    """Check L7: a row count that items does not divide, a target batch size that is neither 1 nor items, a sample-rate mismatch and
    (on the device) CPU tensors raise before any launch."""
    import pytest

    x = torch.zeros(4, 2, n, device=dev)
    prof2, prof3 = (type(loss).Profile(torch.zeros(k, 54, dtype=torch.float64, device=dev), 44100) for k in (2, 3))
    with pytest.raises(ValueError, match="does not divide"):
        loss.pooled(x, prof2, items=3)
    with pytest.raises(ValueError, match="does not divide"):
        loss.profile(x, pool=True, items=3)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="items"):
            loss.pooled(x, prof2, items=bad)
    with pytest.raises(ValueError, match="pool=True"):
        loss.profile(x, items=2)
    with pytest.raises(ValueError, match="batch size"):
        loss.pooled(x, prof3, items=2)
    with pytest.raises(ValueError, match="batch size"):
        loss.pooled(x, torch.zeros(1, 2, n, device=dev), items=2)  # only a profile stands for every item
    with pytest.raises(ValueError, match="Hz"):
        loss.pooled(x, type(loss).Profile(torch.zeros(2, 54, dtype=torch.float64, device=dev), 48000), items=2)
    if torch.device(dev).type != "cpu":
        with pytest.raises(RuntimeError, match="CPU tensor"):
            loss.pooled(x.cpu(), prof2, items=2)
        with pytest.raises(RuntimeError, match="CPU tensor"):
            loss.profile(x.cpu(), pool=True, items=2)
