"""The shared cases of the linked-rows tests: the step in which rows of the track segment share one set of logits and the follower of
a stereo pair carries the mirrored pan (``mst_logit_adam_init_linked`` / ``_step_linked``):
tests/test_online_links_hostsim.py on the host simulator, tests/test_online_links_gpu.py on the device.

TEST INFRASTRUCTURE.  Defined here once so that the two files cannot drift apart.  The driver, guard regions, gradient streams, bounds
and the unlinked sessions are those of tests/online_ref.py, tests/online_best_ref.py, tests/online_sections_ref.py and
tests/online_sections_batch_ref.py, imported unchanged:

* ``LinkedSession``: the two new entry points on ``online_sections_batch_ref.SectionsBatchSession``'s guarded buffers.
* ``linked_f64`` / ``linked_torch``: the float64 restatement and ``torch.optim.Adam`` on the LEADER rows only, behind a gather with a
  sign flip, ``torch.sigmoid`` and a loss that is linear in p with the recorded gradient stream.
* the bound is online_ref's: e(kernel) <= SLACK e(torch fp32) + floor, SLACK = 3, FLOOR = 2^-24.
"""
import functools

import torch

import online_best_ref as B
import online_ref as O
import online_sections_batch_ref as Q
import online_sections_ref as P

COLS, PAN = 27, 25  # the track tensor's columns; ("stereo_panner", "pan")
MAPS = {
    "pair_and_two": [0, 0, 2, 3],
    "two_pairs": [0, 0, 2, 2],
    "middle_pairs": [0, 1, 1, 3, 3],
    "five_pairs": [0, 0, 2, 2, 4, 4, 6, 6, 8, 8],  # 270 coordinates: crosses the loop of the 256-lane workgroup
}


def counts_of(rows):
    return (rows * COLS, 25, 26)


def make_links(leaders, cols=COLS, mirror_col=PAN, segment=0, rows=None):
    from mst import _cabi

    out = _cabi.LogitAdamLinks(segment=segment, rows=len(leaders) if rows is None else rows, cols=cols, mirror_col=mirror_col)
    for r, l in enumerate(leaders):
        out.leader[r] = l
    return out


def sign_of(leaders, mirror_col=PAN, cols=COLS):
    """(rows, cols) of +1, and -1 where a follower carries minus its leader's logit."""
    sign = torch.ones(len(leaders), cols, dtype=torch.float64)
    if mirror_col >= 0:
        for r, l in enumerate(leaders):
            if l != r:
                sign[r, mirror_col] = -1.0
    return sign


def linked_start(theta0, leaders, mirror_col=PAN):
    """What the init launch makes of a start point (segment 0 flat (rows * 27,)): the followers take their leaders' rows."""
    th = theta0[0].view(len(leaders), COLS)
    full = th[torch.tensor(leaders)] * sign_of(leaders, mirror_col).to(th.dtype)
    return [full.reshape(-1).contiguous()] + [t.clone() for t in theta0[1:]]


class LinkedSession(Q.SectionsBatchSession):
    """``online_sections_batch_ref.SectionsBatchSession`` whose two calls are the linked ones, with ``links`` (a ``LogitAdamLinks``)."""

    def __init__(self, drv, theta0, sections, n_iters, n_terms, links, best=False):
        from mst import _cabi

        self.drv, self.cabi, self.sections, self.links = drv, _cabi, sections, links
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
            self.best = B._zeroed_best(drv, words).view(self.items, B.best_words(self.n))
        self.n_terms, self.calls = n_terms, 0
        drv.lib.mst_logit_adam_init_linked(self._segments([None] * len(self.counts)), len(self.counts), self.items, sections, links,
                                           self.state, drv.stream_ptr())
        assert not bool(self.state.cpu().any()), "state not zeroed"

    def step(self, grads, terms, lr, min_delta=0.0, patience=0, betas=O.BETAS, eps=O.EPS):
        assert tuple(terms.shape) == (self.items, self.n_terms) and terms.is_contiguous()
        for g, c in zip(grads, self.counts):
            assert g is None or (tuple(g.shape) == (self.items, self.sections, c) and g.is_contiguous())
        self.drv.lib.mst_logit_adam_step_linked(self._segments(grads), len(self.counts), self.items, self.sections, self.links, terms,
                                                self.n_terms, self.history[self.calls], lr, betas[0], betas[1], eps, min_delta,
                                                patience, self.state, self.best, self.drv.stream_ptr())
        self.calls += 1

    def item_theta(self, b):
        return [t.view(self.items, -1)[b].cpu().clone() for t in self.theta]


# ---- the two references -----------------------------------------------------------------------------------------------------------------
def linked_f64(theta0, stream, leaders, lr, mirror_col=PAN, betas=O.BETAS, eps=O.EPS):
    """The float64 restatement: Adam on the leader rows; every member's chained gradient, signed, added to its leader's.  ``stream``
    per segment (steps, sections, count); -> the full logits per segment."""
    b1, b2 = betas
    sign = sign_of(leaders, mirror_col)
    lead = sorted(set(leaders))
    pos = torch.tensor([lead.index(l) for l in leaders])
    th = [theta0[0].double().view(len(leaders), COLS)[lead].clone()] + [t.double().clone() for t in theta0[1:]]
    m = [torch.zeros_like(t) for t in th]
    v = [torch.zeros_like(t) for t in th]
    steps = stream[0].shape[0]
    for k in range(steps):
        t = k + 1
        for s, dps in enumerate(stream):
            d = dps[k].double().sum(dim=0)
            if s == 0:
                full = th[0][pos] * sign
                p = torch.sigmoid(full)
                g_rows = d.view(len(leaders), COLS) * p * (1.0 - p) * sign
                g = torch.zeros_like(th[0]).index_add_(0, pos, g_rows)
            else:
                p = torch.sigmoid(th[s])
                g = d * p * (1.0 - p)
            m[s] = m[s] + (1.0 - b1) * (g - m[s])
            v[s] = b2 * v[s] + (1.0 - b2) * g * g
            th[s] = th[s] - lr / (1.0 - b1 ** t) * m[s] / (v[s].sqrt() / (1.0 - b2 ** t) ** 0.5 + eps)
    return [(th[0][pos] * sign).reshape(-1)] + th[1:]


def linked_torch(theta0, stream, leaders, lr, mirror_col=PAN, betas=O.BETAS, eps=O.EPS):
    """torch.optim.Adam on the leader rows only, fp32 on the host: a gather with a sign flip, torch.sigmoid, the parameters repeated
    over the sections by ``expand`` and a loss that is linear in p with the recorded gradients."""
    sign = sign_of(leaders, mirror_col).float()
    lead = sorted(set(leaders))
    pos = torch.tensor([lead.index(l) for l in leaders])
    th = [theta0[0].float().view(len(leaders), COLS)[lead].clone().requires_grad_(True)] + [t.float().clone().requires_grad_(True)
                                                                                           for t in theta0[1:]]
    opt = torch.optim.Adam(th, lr=lr, betas=betas, eps=eps, foreach=False)
    steps, sections = stream[0].shape[:2]
    for k in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = 0.0
        for s, dps in enumerate(stream):
            full = (th[0][pos] * sign).reshape(-1) if s == 0 else th[s]
            p = torch.sigmoid(full).unsqueeze(0).expand(sections, -1)
            loss = loss + (p * dps[k]).sum()
        loss.backward()
        opt.step()
    return [(th[0].detach()[pos] * sign).reshape(-1)] + [t.detach() for t in th[1:]]


@functools.lru_cache(maxsize=None)
def references(name, sections, steps, seed=0):
    """(theta_0 as drawn, the linked start, stream, theta_f64, e(torch fp32), floor, lr) of a map: computed once, shared, never
    modified."""
    leaders = MAPS[name]
    counts, lr = counts_of(len(leaders)), 1e-3
    theta0 = O.start(counts, 1e-3, seed)
    stream = P.section_streams(counts, steps, sections, seed=500 + seed)
    start = linked_start(theta0, leaders)
    t64 = linked_f64(theta0, stream, leaders, lr)
    e_torch = O.e_stat(linked_torch(theta0, stream, leaders, lr), t64, start)
    return theta0, start, stream, t64, e_torch, O.floor_term(t64, start), lr


# ---- the invariants -----------------------------------------------------------------------------------------------------------------------
SIGN_BIT = -2 ** 31


def assert_invariants(drv, ses, leaders, tag, mirror_col=PAN):
    """A follower's logits are its leader's bits, the exact negation at the mirrored column; every p is opt_sigmoid of its own logit
    (the plain init kernel's bits), equal in all section rows; followers' moment words are zero; the guards are intact."""
    rows = len(leaders)
    flip = torch.zeros(rows, COLS, dtype=torch.int32)
    if mirror_col >= 0:
        for r, l in enumerate(leaders):
            if l != r:
                flip[r, mirror_col] = SIGN_BIT
    followers = torch.tensor([l != r for r, l in enumerate(leaders)])
    for b in range(ses.items):
        th = ses.theta[0].view(ses.items, rows, COLS)[b].cpu()
        assert torch.equal(O.bits(th), O.bits(th[torch.tensor(leaders)]) ^ flip), f"{tag}: item {b}: a follower's logits are not its leader's"
        one = O.Session(drv, [th.reshape(-1)], 1, 1)  # p = opt_sigmoid(theta) by the plain init kernel
        want = one.p[0].cpu()
        got = ses.rows(0, b).cpu()
        for r in range(ses.sections):
            assert torch.equal(O.bits(got[r]), O.bits(want)), f"{tag}: item {b}: p is not opt_sigmoid of the member's own logit in row {r}"
        if mirror_col < 0:
            p2 = got[0].view(rows, COLS)
            assert torch.equal(O.bits(p2), O.bits(p2[torch.tensor(leaders)]))
        else:
            keep = torch.ones(COLS, dtype=torch.bool)
            keep[mirror_col] = False
            p2 = got[0].view(rows, COLS)
            assert torch.equal(O.bits(p2[:, keep]), O.bits(p2[torch.tensor(leaders)][:, keep])), f"{tag}: a follower's p is not its leader's"
        st = ses.state[b].cpu()
        n0 = rows * COLS
        for moments in (st[O.HDR:O.HDR + n0], st[O.HDR + ses.n:O.HDR + ses.n + n0]):
            assert not bool(moments.view(rows, COLS)[followers].any()), f"{tag}: item {b}: a follower's moment word was written"
    drv.check_guards()


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def check_identity_is_sections_batch(drv, items, sections, rows, best, steps=Q.STEPS, lr=1e-3):
    """Case 1: a map in which every row leads itself is mst_logit_adam_init_sections_batch / _step_sections_batch, bit for bit, in theta,
    every row of p, the state blocks, the history and the best blocks."""
    counts = counts_of(rows)
    theta0 = [O.start(counts, 1e-3, 60 + b) for b in range(items)]
    streams = Q.item_section_streams(counts, steps, items, sections, seed=600)
    terms = Q.item_terms(items, steps, 2, seed=47)
    dev = drv.device
    plain = Q.SectionsBatchSession(drv, theta0, sections, steps, 2, best=best)
    ses = LinkedSession(drv, theta0, sections, steps, 2, make_links(list(range(rows))), best=best)
    up, tm = Q.stacked(streams, dev), terms.to(dev).contiguous()
    extra = (0.01, 4) if best else ()
    for k in range(-1, steps):
        if k >= 0:
            plain.step([u[k] for u in up], tm[k], lr, *extra)
            ses.step([u[k] for u in up], tm[k], lr, *extra)
        if k % 7 == 0 or k in (-1, steps - 1):  # after the init, and a difference never heals
            for a, b_ in zip(ses.theta + ses.p, plain.theta + plain.p):
                assert B.same(a, b_), f"identity map, step {k}: theta or p differs from the sections-batch call"
            assert torch.equal(ses.state.cpu(), plain.state.cpu()), f"identity map, step {k}: state differs"
            assert B.same(ses.history[:k + 1], plain.history[:k + 1])
            if best:
                assert torch.equal(ses.best.cpu(), plain.best.cpu()), f"identity map, step {k}: best block differs"
    drv.check_guards()
    if not best:
        for b in range(items):
            assert ses.words(b) == (steps, 0, 0, steps)


def check_parity(drv, name, sections, steps, record=None):
    """Case 2: a whole stream through the kernel, the float64 restatement and torch in fp32 on the leader rows; the invariants hold
    after every step."""
    leaders = MAPS[name]
    theta0, start, stream, t64, e_torch, floor, lr = references(name, sections, steps)
    ses = LinkedSession(drv, [theta0], sections, steps, 1, make_links(leaders))
    assert_invariants(drv, ses, leaders, f"{name}, after the init")
    for got, want in zip(ses.item_theta(0), start):
        assert B.same(got, want), "the init did not give the followers their leaders' logits"
    dev = drv.device
    up, term = [s.to(dev).contiguous() for s in stream], torch.ones(1, 1, device=dev)
    for k in range(steps):
        ses.step([u[k:k + 1] for u in up], term, lr)
        assert_invariants(drv, ses, leaders, f"{name}, step {k}")
    got = ses.item_theta(0)
    e_kernel = O.e_stat(got, t64, start)
    print(f"\n[linked logit-Adam {name}, {sections} section(s), {steps} steps] e(kernel) = {e_kernel:.3e}, e(torch fp32) = {e_torch:.3e}, "
          f"floor {floor:.3e}")
    if record is not None:
        record(kernel=e_kernel, torch_fp32=e_torch, floor=floor)
    assert ses.words(0) == (steps, 0, 0, steps)
    assert bool((torch.cat(got) != torch.cat(start)).any())
    assert e_kernel <= O.SLACK * e_torch + floor


def check_zero_logits_pan_centre(drv):
    """Case 3: at theta = 0 the leader's and the follower's pan are both 0.5, and -0.0 is what the follower carries."""
    leaders = MAPS["pair_and_two"]
    theta0 = [torch.zeros(c) for c in counts_of(len(leaders))]
    ses = LinkedSession(drv, [theta0], 2, 1, 1, make_links(leaders))
    p = ses.rows(0, 0).cpu().view(2, len(leaders), COLS)
    assert bool((p == 0.5).all())
    th = ses.theta[0].cpu().view(len(leaders), COLS)
    assert O.bits(th)[1, PAN].item() == SIGN_BIT and not bool(O.bits(th)[0].any())
    assert_invariants(drv, ses, leaders, "theta = 0")


def check_nonfinite_follower(drv, where, at=3, steps=6, items=3, sections=2):
    """Case 4: a NaN in a FOLLOWER row's gradient only, or finite members whose group sum overflows, in item 1 of 3 at step 3 of 6:
    item 1's iteration changes nothing and is the one reported; items 0 and 2 are bit for bit a run without the fault."""
    if where == "nan":
        leaders, mirror = MAPS["pair_and_two"], PAN
    else:  # g <= d / 4 < 8.6e37: only a group of five or more can overflow, which a mirrored pan does not take
        leaders, mirror = [0, 0, 0, 0, 0, 0], -1
    rows = len(leaders)
    counts, lr = counts_of(rows), 1e-3
    theta0 = [O.start(counts, 1e-3, 70 + b) for b in range(items)]
    streams = Q.item_section_streams(counts, steps, items, sections, seed=700)
    terms = Q.item_terms(items, steps, 2, seed=48)
    dev = drv.device

    def run(streams):
        ses = LinkedSession(drv, theta0, sections, steps, 2, make_links(leaders, mirror_col=mirror))
        up, tm = Q.stacked(streams, dev), terms.to(dev).contiguous()
        snaps = []
        for k in range(steps):
            ses.step([u[k] for u in up], tm[k], lr)
            snaps.append([ses.everything(b) for b in range(items)])
        return ses, snaps

    clean, clean_snaps = run(streams)
    faulty = [[s.clone() for s in item] for item in streams]
    if where == "nan":
        faulty[1][0][at, 1, 1 * COLS + 7] = float("nan")  # row 1 follows row 0
    else:
        faulty[1][0][at, :, 4::COLS] = 1.6e38  # column 4 of every row: d = 3.2e38 per member, g about 8e37, six of them
        assert bool(torch.isfinite(P.host_sum(faulty[1][0][at])).all())
    ses, snaps = run(faulty)
    drv.check_guards()
    for part in (0, 1):
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
    assert_invariants(drv, ses, leaders, f"after a {where} fault", mirror_col=mirror)


def check_null_gradient(drv, which, items=2, sections=2, steps=6):
    """Case 5: a NULL-gradient segment keeps theta, the moments and all rows of p - another segment (1) or the tied one itself (0) -
    while the others move."""
    leaders = MAPS["two_pairs"]
    counts, lr = counts_of(len(leaders)), 1e-3
    theta0 = [O.start(counts, 1e-3, 80 + b) for b in range(items)]
    streams = Q.item_section_streams(counts, steps, items, sections, seed=800)
    dev = drv.device
    ses = LinkedSession(drv, theta0, sections, steps, 1, make_links(leaders))
    th0, p0 = ses.theta[which].clone(), ses.p[which].clone()
    other0 = ses.theta[2].clone()
    up, term = Q.stacked(streams, dev), torch.ones(items, 1, device=dev)
    for k in range(steps):
        ses.step([None if s == which else u[k] for s, u in enumerate(up)], term, lr)
    assert B.same(ses.theta[which], th0) and B.same(ses.p[which], p0)
    assert not B.same(ses.theta[2], other0)
    lo = sum(counts[:which])
    hi = lo + counts[which]
    for b in range(items):
        st = ses.state[b].cpu()
        m, v = st[O.HDR:O.HDR + ses.n], st[O.HDR + ses.n:]
        assert not bool(m[lo:hi].any()) and not bool(v[lo:hi].any()) and bool(m[hi:].any()) and bool(v[hi:].any())
        assert ses.words(b) == (steps, 0, 0, steps)
    assert_invariants(drv, ses, leaders, f"NULL gradient in segment {which}")


def check_best_snapshot(drv, items=2, sections=2):
    """Case 6: the best block holds the logits BEFORE the update of the iteration that improved - for every member - and follows
    online_best_ref's scripted sequence (min_delta 0.25, patience 2: best at 1, settled at 3)."""
    leaders = MAPS["middle_pairs"]
    counts = counts_of(len(leaders))
    losses = list(B.SEQUENCE)
    steps = len(losses)
    theta0 = [O.start(counts, 1e-3, 90 + b) for b in range(items)]
    streams = Q.item_section_streams(counts, steps, items, sections, seed=900)
    dev = drv.device
    ses = LinkedSession(drv, theta0, sections, steps, 1, make_links(leaders), best=True)
    up = Q.stacked(streams, dev)
    tm = torch.tensor(losses, dtype=torch.float32).view(steps, 1, 1).expand(steps, items, 1).contiguous().to(dev)
    before = []
    for k in range(steps):
        before.append([torch.cat(ses.item_theta(b)) for b in range(items)])
        ses.step([u[k] for u in up], tm[k], B.LR, 0.25, 2)
    assert B.replay(losses, 0.25, 2) == (1, 3.0, 2, 3)
    rows = len(leaders)
    flip = O.bits(sign_of(leaders).float()) & SIGN_BIT  # the sign bit where a follower is mirrored
    for b in range(items):
        block = ses.best[b].cpu()
        assert block[:4].tolist()[0] == 1 + 1 and block[3].item() == 3 + 1
        stored = block[B.BEST_HDR:B.BEST_HDR + ses.n].view(torch.float32)
        assert B.same(stored, before[1][b]), f"item {b}: the best block is not the iterate the loss was evaluated at"
        tracks = O.bits(stored[:rows * COLS]).view(rows, COLS)
        assert torch.equal(tracks, tracks[torch.tensor(leaders)] ^ flip), f"item {b}: the best block's members disagree"
        assert ses.words(b) == (4, 0, 0, steps)
    assert_invariants(drv, ses, leaders, "best")


def check_items_are_single_sessions(drv, best, name="five_pairs", items=3, sections=2, steps=Q.STEPS, lr=1e-3):
    """Case 7: every item of a 3-item batch is bit for bit a single-item linked session."""
    leaders = MAPS[name]
    counts = counts_of(len(leaders))
    theta0 = [O.start(counts, 1e-3, 110 + b) for b in range(items)]
    streams = Q.item_section_streams(counts, steps, items, sections, seed=1100)
    terms = Q.item_terms(items, steps, 2, seed=49)
    dev = drv.device
    links = make_links(leaders)
    ses = LinkedSession(drv, theta0, sections, steps, 2, links, best=best)
    alone = [LinkedSession(drv, [theta0[b]], sections, steps, 2, links, best=best) for b in range(items)]
    up, tm = Q.stacked(streams, dev), terms.to(dev).contiguous()
    extra = (0.01, 4) if best else ()
    for k in range(steps):
        ses.step([u[k] for u in up], tm[k], lr, *extra)
        for b, one in enumerate(alone):
            one.step([u[k, b:b + 1] for u in up], tm[k, b:b + 1], lr, *extra)
        if k % 7 == 0 or k == steps - 1:
            for b, one in enumerate(alone):
                mine, theirs = ses.everything(b), one.everything(0)
                for x, y in zip(mine, theirs):
                    assert (x is None and y is None) or torch.equal(O.bits(x), O.bits(y)), f"item {b}, step {k}: not the single session"
                assert B.same(ses.history[:k + 1, b], one.history[:k + 1, 0])
    assert_invariants(drv, ses, leaders, "three items")
    assert not B.same(ses.theta[0].view(items, -1)[0], ses.theta[0].view(items, -1)[1])


def check_refusals(drv):
    """Case 8: a NULL map, rows 0 and 257, rows * cols off the segment's per-item count, a leader that points forward or does not lead
    itself, mirror_col outside [-1, cols), a segment that is not there, and bad arguments of the sections-batch calls launch nothing and
    write nothing."""
    from mst import _cabi

    L, st = drv.lib, drv.stream_ptr()
    for name in ("mst_logit_adam_init_linked", "mst_logit_adam_step_linked"):
        assert hasattr(L, name) and name in _cabi.SIGNATURES
    assert L.mst_abi_version() == _cabi.ABI_VERSION == 13 and _cabi.OPT_MAX_LINK_ROWS == 256
    items, sections, rows, cols = 2, 2, 4, 3
    c = rows * cols
    theta, row, term = drv.guarded(items * c), drv.guarded(items * 2), drv.guarded(items)
    p, grad = drv.guarded(items * sections * c), drv.guarded(items * sections * c)
    state, best = drv.guarded(items * (O.HDR + 2 * c)), drv.guarded(items * B.best_words(c))
    seg = (_cabi.LogitAdamSegment * 1)()
    seg[0].theta, seg[0].p, seg[0].grad_p, seg[0].count = theta.data_ptr(), p.data_ptr(), grad.data_ptr(), items * c

    def refused(fn, *args):
        try:
            fn(*args)
        except _cabi.AbiError as e:
            assert e.code != 0
            return
        raise AssertionError(f"{fn.__name__} accepted {args}")

    good_links = dict(leaders=[0, 0, 2, 2], cols=cols, mirror_col=1, segment=0, rows=None)
    good = dict(items=items, S=sections, n_seg=1, state=state, best=None, lr=1e-3, n_terms=1)

    def both(links=None, null=False, **change):
        a = dict(good, **change)
        k = None if null else make_links(**dict(good_links, **(links or {})))
        refused(L.mst_logit_adam_init_linked, seg, a["n_seg"], a["items"], a["S"], k, a["state"], st)
        refused(L.mst_logit_adam_step_linked, seg, a["n_seg"], a["items"], a["S"], k, term, a["n_terms"], row, a["lr"], 0.9, 0.999, 1e-8,
                0.0, 0, a["state"], a["best"], st)

    both(null=True)
    big = list(range(256))
    for links in (dict(leaders=[], rows=0), dict(leaders=big, rows=257), dict(leaders=[], rows=-1), dict(leaders=[0, 0, 2]),
                  dict(leaders=[0, 0, 2, 2, 4]), dict(cols=4), dict(cols=0), dict(leaders=[0, 2, 2, 2]), dict(leaders=[1, 1, 2, 2]),
                  dict(leaders=[0, 0, 1, 2]), dict(leaders=[0, 0, 2, 200]), dict(mirror_col=cols), dict(mirror_col=-2), dict(segment=1),
                  dict(segment=-1)):
        both(links)
    for change in (dict(items=0), dict(items=1025), dict(items=3), dict(S=0), dict(S=65), dict(n_seg=0), dict(state=None),
                   dict(state=state.data_ptr() + 2)):
        both(**change)
    for change in (dict(lr=0.0), dict(n_terms=0), dict(n_terms=9), dict(best=best.data_ptr() + 2)):
        a = dict(good, **change)
        refused(L.mst_logit_adam_step_linked, seg, 1, items, sections, make_links(**good_links), term, a["n_terms"], row, a["lr"], 0.9,
                0.999, 1e-8, 0.0, 0, state, a["best"], st)
    for t in (theta, p, grad, row, term, state, best):
        assert bool(torch.isnan(t).all()), "a refused call wrote something"
    drv.check_guards()
