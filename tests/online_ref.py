"""The reference of the logit-Adam tests (tests/test_online_hostsim.py on the host simulator, tests/test_online_gpu.py on the device).

TEST INFRASTRUCTURE.  Defined here once so that the two files cannot drift apart:

* ``adam_f64``: a float64 restatement of the recurrence ``mst_logit_adam_step`` documents (include/diffmst_hip.h).
* ``adam_torch``: ``torch.optim.Adam`` (single-tensor path, defaults) behind ``torch.sigmoid`` in fp32 on the host - the computation
  the reference's scripts/online.py runs around its console.
* ``gradient_stream``: a seeded stream of dL/dp that does not depend on theta, so that trajectories differ by rounding only:
  per-coordinate scales 10^U(-6, 2), biased so that parameters drift, a few coordinates always zero, a few zero from half way.
* ``e_stat`` / ``bound``: e(x) = |theta_x - theta_f64| / |theta_f64 - theta_0| at the last step and the three-way form of
  tests/ctrl_ref.py, e(kernel) <= 3 e(torch fp32) + 2^-24 |theta_f64| / |theta_f64 - theta_0|.
* ``Driver`` / ``Session``: the C ABI on NaN-filled buffers with guard regions on either side, on the host (simulator library) or on
  the device (product library); and the cases themselves, ``check_*``, which both files call.
"""
import ctypes
import functools

import torch

GUARD = 64
SLACK = 3.0            # what the controller tests grant a second correct fp32 evaluation
FLOOR = 2.0 ** -24     # half an ulp of the float64 result rounded to fp32
BETAS, EPS = (0.9, 0.999), 1e-8
SIGMOID_MARGIN_ULP = 2.0  # a different exp
HDR = 16               # int32 words in front of the moments (include/diffmst_hip.h)

# name -> (segment counts, steps, lr, scale of theta_0)
STREAMS = {
    "song3": ((81, 25, 26), 50, 1e-3, 1e-3),
    "song16": ((432, 25, 26), 200, 1e-2, 1e-3),
    "tails": ((200,), 50, 1e-3, 3.0),  # sigmoid tails
}
TAIL_COUNTS = (1, 63, 64, 65, 1025)  # lane tails and the loop of the 256-lane workgroup


# ---- construction ---------------------------------------------------------------------------------------------------------------
def gradient_stream(counts, steps, seed):
    """-> [per segment: (steps, count) fp32], the same numbers for every evaluation."""
    g = torch.Generator().manual_seed(seed)
    n = sum(counts)
    scale = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 8.0 - 6.0)
    bias = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    dp = scale * (bias + 0.5 * torch.randn(steps, n, generator=g, dtype=torch.float64))
    perm = torch.randperm(n, generator=g)
    k = min(3, n // 4)
    zero, half = perm[:k], perm[k:2 * k]
    dp[:, zero] = 0.0
    dp[steps // 2:, half] = 0.0
    return list(dp.float().split(list(counts), dim=1)), zero, half


def start(counts, scale, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return [scale * torch.randn(c, generator=g) for c in counts]


# ---- the two references ---------------------------------------------------------------------------------------------------------
def adam_f64(theta0, stream, lr, betas=BETAS, eps=EPS):
    """The recurrence in float64; a segment whose stream is None keeps its logits."""
    b1, b2 = betas
    th = [t.double().clone() for t in theta0]
    m = [torch.zeros_like(t) for t in th]
    v = [torch.zeros_like(t) for t in th]
    steps = next(s.shape[0] for s in stream if s is not None)
    for k in range(steps):
        t = k + 1
        for s, dps in enumerate(stream):
            if dps is None:
                continue
            p = torch.sigmoid(th[s])
            g = dps[k].double() * p * (1.0 - p)
            m[s] = m[s] + (1.0 - b1) * (g - m[s])
            v[s] = b2 * v[s] + (1.0 - b2) * g * g
            th[s] = th[s] - lr / (1.0 - b1 ** t) * m[s] / (v[s].sqrt() / (1.0 - b2 ** t) ** 0.5 + eps)
    return th


def adam_torch(theta0, stream, lr, betas=BETAS, eps=EPS):
    """torch.optim.Adam behind torch.sigmoid, fp32, on the host."""
    th = [t.float().clone().requires_grad_(True) for t in theta0]
    opt = torch.optim.Adam(th, lr=lr, betas=betas, eps=eps, foreach=False)
    steps = next(s.shape[0] for s in stream if s is not None)
    for k in range(steps):
        opt.zero_grad(set_to_none=True)
        for s, dps in enumerate(stream):
            if dps is not None:
                torch.sigmoid(th[s]).backward(dps[k])
        opt.step()
    return [t.detach() for t in th]


def _cat(ts):
    return torch.cat([t.detach().double().cpu().reshape(-1) for t in ts])


def e_stat(theta, theta64, theta0):
    return float((_cat(theta) - _cat(theta64)).norm() / (_cat(theta64) - _cat(theta0)).norm())


def floor_term(theta64, theta0):
    return FLOOR * float(_cat(theta64).norm() / (_cat(theta64) - _cat(theta0)).norm())


@functools.lru_cache(maxsize=None)
def references(name, seed=0):
    """(theta_0, stream, theta_f64, e(torch fp32), floor) of a named stream: computed once, shared, never modified."""
    counts, steps, lr, scale = STREAMS[name] if name in STREAMS else ((int(name),), 3, 1e-3, 1e-3)
    stream, _, _ = gradient_stream(counts, steps, seed)
    theta0 = start(counts, scale, seed)
    t64 = adam_f64(theta0, stream, lr)
    return theta0, stream, t64, e_stat(adam_torch(theta0, stream, lr), t64, theta0), floor_term(t64, theta0), lr


# ---- the C ABI on guarded buffers -------------------------------------------------------------------------------------------------
class Driver:
    """``lib``: a bound library; ``device``: where its kernels read and write ("cpu" for the simulator)."""

    def __init__(self, lib, device):
        self.lib, self.device = lib, torch.device(device)
        self._all = []

    def guarded(self, n):
        """n fp32 NaNs with GUARD more on either side -> the inner view; ``check_guards`` looks at every buffer handed out."""
        buf = torch.full((n + 2 * GUARD,), float("nan"), device=self.device)
        self._all.append((buf, n))
        return buf[GUARD:GUARD + n]

    def check_guards(self):
        for buf, n in self._all:
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), "written outside a buffer"

    def stream_ptr(self):
        if self.device.type == "cpu":
            return None
        from mst import _hip

        return _hip.current_stream_ptr(self.device)


class Session:
    """One optimiser state over segments that start at ``theta0`` (host tensors)."""

    def __init__(self, drv, theta0, n_iters, n_terms):
        from mst import _cabi

        self.drv, self.cabi = drv, _cabi
        self.counts = [t.numel() for t in theta0]
        self.n = sum(self.counts)
        self.theta = [drv.guarded(c) for c in self.counts]
        for dst, src in zip(self.theta, theta0):
            dst.copy_(src)
        self.p = [drv.guarded(c) for c in self.counts]
        nbytes = drv.lib.mst_logit_adam_state_bytes(self.n)
        assert nbytes == 4 * (HDR + 2 * self.n)
        self.state = drv.guarded(nbytes // 4).view(torch.int32)
        self.history = drv.guarded(n_iters * (1 + n_terms)).view(n_iters, 1 + n_terms)
        self.n_terms, self.calls = n_terms, 0
        drv.lib.mst_logit_adam_init(self._segments([None] * len(theta0)), len(theta0), self.state, drv.stream_ptr())
        assert not bool(self.state.cpu().any()), "state not zeroed"

    def _segments(self, grads):
        seg = (self.cabi.LogitAdamSegment * len(self.counts))()
        for s, th, p, g, c in zip(seg, self.theta, self.p, grads, self.counts):
            s.theta, s.p, s.grad_p, s.count = th.data_ptr(), p.data_ptr(), None if g is None else g.data_ptr(), c
        return seg

    def step(self, grads, terms, lr, betas=BETAS, eps=EPS):
        """grads: per segment a (count,) fp32 tensor on the driver's device or None; terms: (n_terms,) fp32 on that device."""
        assert terms.numel() == self.n_terms
        ptrs = (ctypes.c_void_p * self.n_terms)(*[terms.data_ptr() + 4 * j for j in range(self.n_terms)])
        row = self.history[self.calls]
        self.drv.lib.mst_logit_adam_step(self._segments(grads), len(self.counts), ptrs, self.n_terms, row, lr, betas[0], betas[1], eps,
                                         self.state, self.drv.stream_ptr())
        self.calls += 1

    def run(self, stream, lr, terms=None):
        """Every step of a stream (host tensors, uploaded once); the loss terms default to one finite number."""
        dev = self.drv.device
        up = [None if s is None else s.to(dev).contiguous() for s in stream]
        steps = next(s.shape[0] for s in stream if s is not None)
        terms = torch.ones(steps, self.n_terms) if terms is None else terms
        terms = terms.to(dev).contiguous()
        for k in range(steps):
            self.step([None if s is None else s[k] for s in up], terms[k], lr)

    def words(self):
        """(t, status, iteration that set it, calls)"""
        return tuple(self.state[:4].cpu().tolist())

    def moments(self):
        st = self.state.cpu()
        return st[HDR:HDR + self.n], st[HDR + self.n:HDR + 2 * self.n]  # as int32 bit patterns

    def thetas(self):
        return [t.cpu().clone() for t in self.theta]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def ulps_from_f64(p, exact):
    """The largest |p - exact| in ulps of fl32(exact): p fp32, exact float64.  (Measured from the float64 value itself, not from its
    rounding: torch's own fp32 sigmoid is 2.11 ulp away on the grid of case 2 by this measure.)"""
    ref = exact.float()
    ulp = torch.nextafter(ref, torch.full_like(ref, float("inf"))).double() - ref.double()
    return ((p.double().cpu() - exact).abs() / ulp).max().item()


def sigmoid_grid():
    return torch.linspace(-20.0, 20.0, 4097, dtype=torch.float64).float()


@functools.lru_cache(maxsize=None)
def sigmoid_bound():
    """Case 2's bound: torch's own fp32 sigmoid's distance on the grid, plus the margin."""
    x = sigmoid_grid()
    return ulps_from_f64(torch.sigmoid(x), torch.sigmoid(x.double())) + SIGMOID_MARGIN_ULP


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def check_parity(drv, name, record=None):
    """Case 1: a whole stream through the kernel, the float64 recurrence and torch in fp32."""
    theta0, stream, t64, e_torch, floor, lr = references(name)
    ses = Session(drv, theta0, stream[0].shape[0], 1)
    ses.run(stream, lr)
    drv.check_guards()
    got = ses.thetas()
    for th, p in zip(got, ses.p):
        assert bool(torch.isfinite(th).all()) and bool(torch.isfinite(p.cpu()).all()), "logits or parameters not fully written"
    e_kernel = e_stat(got, t64, theta0)
    print(f"\n[logit-Adam {name}] e(kernel) = {e_kernel:.3e}, e(torch fp32) = {e_torch:.3e}, floor {floor:.3e}")
    if record is not None:
        record(kernel=e_kernel, torch_fp32=e_torch, floor=floor)
    assert ses.words() == (stream[0].shape[0], 0, 0, stream[0].shape[0])
    assert e_kernel <= SLACK * e_torch + floor
    return ses


def check_sigmoid(drv, record=None):
    """Case 2: p = sigmoid(theta) as mst_logit_adam_init writes it."""
    x = sigmoid_grid()
    ses = Session(drv, [x], 1, 1)
    drv.check_guards()
    p = ses.p[0].cpu()
    assert bool((p[1:] >= p[:-1]).all()), "not monotone"
    exact = torch.sigmoid(x.double())
    mine, theirs = ulps_from_f64(p, exact), sigmoid_bound() - SIGMOID_MARGIN_ULP
    print(f"\n[sigmoid on 4097 points of [-20, 20]] kernel {mine:.2f} ulp, torch fp32 {theirs:.2f} ulp")
    if record is not None:
        record(kernel_ulp=mine, torch_ulp=theirs)
    assert mine <= sigmoid_bound()
    edge = torch.tensor([0.0, -0.0, 88.0, -88.0, 104.0, -104.0])
    pe = Session(drv, [edge], 1, 1).p[0].cpu()
    drv.check_guards()
    assert bool(torch.isfinite(pe).all()) and bool((pe >= 0).all()) and bool((pe <= 1).all())


def check_unchanged_bits(drv):
    """Case 3: a NULL-gradient segment and the all-zero-gradient coordinates keep theta, m and v bit for bit over 10 steps."""
    counts, lr = (81, 25, 26), 1e-3
    stream, zero, _ = gradient_stream(counts, 10, 3)
    assert len(zero) == 3
    theta0 = start(counts, 1e-3, 3)
    stream[1] = None
    ses = Session(drv, theta0, 10, 1)
    p0 = [p.cpu().clone() for p in ses.p]
    ses.run(stream, lr)
    drv.check_guards()
    got = ses.thetas()
    m, v = ses.moments()
    assert torch.equal(bits(got[1]), bits(theta0[1])) and torch.equal(bits(ses.p[1]), bits(p0[1]))
    assert not bool(m[81:106].any()) and not bool(v[81:106].any())
    flat, flat0 = torch.cat(got), torch.cat(theta0)
    assert torch.equal(bits(flat[zero]), bits(flat0[zero]))
    assert not bool(m[zero].any()) and not bool(v[zero].any())
    t64 = adam_f64(theta0, stream, lr)  # the other segments move as in case 1
    assert e_stat(got, t64, theta0) <= SLACK * e_stat(adam_torch(theta0, stream, lr), t64, theta0) + floor_term(t64, theta0)
    assert ses.words() == (10, 0, 0, 10)


def check_nonfinite(drv, where):
    """Case 4: one NaN in a gradient, or an Inf loss term, at step 3 of 6: that step changes nothing and is the one reported."""
    counts, lr = (81, 25, 26), 1e-3
    stream, _, _ = gradient_stream(counts, 6, 4)
    stream = [s.clone() for s in stream]
    terms = torch.rand(6, 2, generator=torch.Generator().manual_seed(4))
    if where == "gradient":
        stream[2][3, 7] = float("nan")
    else:
        terms[3, 1] = float("inf")
    theta0 = start(counts, 1e-3, 4)
    ses = Session(drv, theta0, 6, 2)
    dev = drv.device
    snaps = []
    for k in range(6):
        ses.step([s[k].to(dev) for s in stream], terms[k].to(dev), lr)
        snaps.append((torch.cat(ses.thetas()), *[x.clone() for x in ses.moments()], torch.cat([p.cpu() for p in ses.p])))
    drv.check_guards()
    for a, b in zip(snaps[3], snaps[2]):
        assert torch.equal(bits(a), bits(b)), "the rejected step changed something"
    assert not torch.equal(bits(snaps[4][0]), bits(snaps[3][0])), "the step after it did not move"
    assert bool(torch.isfinite(snaps[5][0]).all())
    assert ses.words() == (5, 1, 3, 6)
    h = ses.history.cpu()
    assert torch.equal(bits(h[:, 1:]), bits(terms)), "a history row was not written"
    assert torch.equal(bits(h[:, 0]), bits(terms[:, 0] + terms[:, 1]))
    # what was applied is Adam on the five other gradients
    clean = [torch.cat([s[:3], s[4:]]) for s in stream]
    t64 = adam_f64(theta0, clean, lr)
    assert e_stat(ses.thetas(), t64, theta0) <= SLACK * e_stat(adam_torch(theta0, clean, lr), t64, theta0) + floor_term(t64, theta0)


def check_history(drv, n_terms):
    """Case 5: every row is the terms and their left-to-right fp32 sum from zero, bit for bit."""
    g = torch.Generator().manual_seed(5 + n_terms)
    steps = 4
    terms = (torch.randn(steps, n_terms, generator=g) * 10.0 ** torch.randint(-4, 4, (steps, n_terms), generator=g)).float()
    stream, _, _ = gradient_stream((65,), steps, 5)
    ses = Session(drv, start((65,), 1e-3, 5), steps, n_terms)
    ses.run(stream, 1e-3, terms)
    drv.check_guards()
    total = torch.zeros(steps)
    for j in range(n_terms):
        total = total + terms[:, j]  # the script's `loss = 0; loss += value`
    h = ses.history.cpu()
    assert torch.equal(bits(h[:, 1:]), bits(terms)) and torch.equal(bits(h[:, 0]), bits(total))
