"""Best-iterate fits on the MI355X: the cases of tests/test_online_best_hostsim.py on the device (through the C ABI of the product
library, tests/online_best_ref.py), then ``mst.online.optimize`` / ``optimize_batch`` with ``keep_best``, ``patience`` and
``poll_every`` end to end - the report against a numpy-fp32 replay of the returned history, the returned logits, mix and dictionaries
against what a capturing callback and a recording loss saw at that iteration, the plain calls bit for bit what they were, no host wait
inside the loop, ``pick`` / ``best_of`` into ``render_blocks`` - and the errors.  Songs and shapes are those of
tests/test_online_gpu.py (T = 3, N = 32768, 20 iterations).

The losses get one more term, ``bump[n] + 0.0 * mix.sum()``: a differentiable one-element (or ``(B,)``) device tensor whose gradient is
zero, so the fit is the one without it, while the loss the kernel ranks is scripted from outside: the best iterate is not the last one
by construction, and an item settles where the script says."""
import functools

import pytest
import torch

import online_batch_ref as B
import online_best_ref as R
import online_ref as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, ITERS = 1e-3, 20
BIG = 1.0e6  # far above any loss of these songs: an iteration that carries it cannot improve


@pytest.fixture()
def drv():
    from mst import _hip

    d = O.Driver(_hip.lib(), DEV)
    yield d
    B.scrub(d)  # the NaN-filled buffers go back to the allocator as zeros


# ---- the kernels through the C ABI: the simulator's cases -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["song3", "tails"])
def test_the_fit_is_the_plain_steps(drv, name):
    R.check_does_not_perturb(drv, name)


def test_scripted_sequence(drv):
    R.check_scripted_sequence(drv)


def test_a_tie_keeps_the_earlier_iterate(drv):
    R.check_ties(drv)


@pytest.mark.parametrize("where", ["gradient", "loss"])
def test_nonfinite_input_leaves_the_best_block_alone(drv, where):
    R.check_nonfinite(drv, where)


def test_null_gradient_segment_is_in_the_snapshot(drv):
    R.check_null_gradient(drv)


@pytest.mark.parametrize("items", [3, 8])
def test_every_item_is_an_independent_best_session(drv, items):
    R.check_batch(drv, items)


@pytest.mark.parametrize("count", O.TAIL_COUNTS)
def test_lane_tails_and_the_guards_of_the_best_block(drv, count):
    R.check_lane_tails(drv, count)


def test_unsupported_arguments_launch_nothing(drv):
    R.check_refusals(drv)


# ---- optimize(keep_best=True) end to end ------------------------------------------------------------------------------------------
class Bumped:
    """AudioFeatureLoss with a sixth term scripted from outside, recording the mix it is handed.  ``bump``: (n_iters,) for ``optimize``,
    (n_iters, B) for ``optimize_batch``, on the device."""

    def __init__(self, inner, bump):
        self.inner, self.bump, self.mixes = inner, bump, []

    def _with_bump(self, out, mix, zero):
        self.mixes.append(mix.detach().clone())
        out = dict(out)
        out["bump"] = self.bump[len(self.mixes) - 1] + zero
        return out

    def __call__(self, mix, target):
        return self._with_bump(self.inner(mix, target), mix, 0.0 * mix.sum())

    def per_item(self, mix, target):
        return self._with_bump(self.inner.per_item(mix, target), mix, 0.0 * mix.sum(dim=(1, 2)))

    def profile(self, ref):
        return self.inner.profile(ref)


def last_five():
    bump = torch.zeros(ITERS)
    bump[-5:] = BIG
    return bump.to(DEV)


@functools.lru_cache(maxsize=None)
def best_run():
    """One captured keep_best run of song 0 whose last five iterations carry the bump; shared and never modified."""
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize

    tracks, ref = G.song(0)
    console, cap, loss = AdvancedMixConsole(44100), G.Capture(), Bumped(AudioFeatureLoss(G.WEIGHTS, 44100), last_five())
    torch.manual_seed(0)
    out = optimize(tracks, ref, console, loss, n_iters=ITERS, lr=LR, callback=cap, keep_best=True)
    return out, cap, console, loss


def test_keep_best_returns_the_best_iterate(record):
    import test_online_gpu as G

    out, cap, console, loss = best_run()
    assert len(out) == 9
    history, report = out[7], out[8]
    assert list(history) == ["loss"] + list(cap.losses[0]) and list(history)[-1] == "bump" and len(history["loss"]) == ITERS
    at, best, _, settled = R.replay(history["loss"])
    print(f"\n[keep_best] best iteration {report.best_iteration} loss {report.best_loss:.6e}; last loss {history['loss'][-1]:.6e}")
    record(best_iteration=report.best_iteration, best_loss=report.best_loss)
    assert (report.best_iteration, report.best_loss, report.settled_at, report.iterations_run) == (at, best, settled, ITERS)
    assert isinstance(report.best_iteration, int) and isinstance(report.best_loss, float) and settled is None
    assert at < ITERS - 5 and at > 0  # not vacuous: neither the last iterate nor the start point
    for got, seen in zip((out[1], out[3], out[5]), cap.logits[at]):
        assert G.same_bits(got, seen)
    assert len(loss.mixes) == ITERS  # finish() runs the console, not the loss
    assert out[0].is_cuda and torch.equal(out[0], loss.mixes[at][0])
    dicts = console._denormalized_dicts(*cap.params[at])
    assert G.same_bits(out[2]["input_fader"]["gain_db"], dicts[0]["input_fader"]["gain_db"])
    assert G.same_bits(out[6]["output_fader"]["gain_db"], dicts[2]["output_fader"]["gain_db"])


def test_keep_best_does_not_perturb_the_fit_and_the_plain_call_is_what_it_was():
    import test_online_gpu as G

    plain, plain_cap, _ = G.captured(0)  # the run tests/test_online_gpu.py replays through the float64 recurrence and torch's Adam
    again, _, _ = G.run(0, capture=False)
    assert len(plain) == len(again) == 8
    assert G.same_bits(again[0], plain[0]) and again[7] == plain[7]
    for i in (1, 3, 5):
        assert G.same_bits(again[i], plain[i])
    assert G.same_bits(again[2]["input_fader"]["gain_db"], plain[2]["input_fader"]["gain_db"])
    assert G.same_bits(again[6]["output_fader"]["gain_db"], plain[6]["output_fader"]["gain_db"])
    # the same trajectory with the best-iterate step: every iteration's logits, parameters and terms
    out, cap, _, _ = best_run()
    for n in range(ITERS):
        for a, b in zip(cap.logits[n] + cap.params[n], plain_cap.logits[n] + plain_cap.params[n]):
            assert G.same_bits(a, b), f"iteration {n}"
    for name, values in plain[7].items():
        if name != "loss":
            assert out[7][name] == values
    assert out[7]["loss"][:ITERS - 5] == plain[7]["loss"][:ITERS - 5]


def test_no_host_wait_inside_the_loop():
    import test_online_gpu as G
    from mst import online
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole

    tracks, ref = G.song(0)
    console, loss = AdvancedMixConsole(44100, validate="deferred"), AudioFeatureLoss(G.WEIGHTS, 44100)
    online.optimize(tracks, ref, console, loss, n_iters=1, keep_best=True)  # the constant tables are built on the first call
    torch.manual_seed(0)
    r = online._Run(tracks, ref, console, loss, 0.001, LR, ITERS, (0.9, 0.999), 1e-8, None, None, {}, keep_best=True, patience=3,
                    min_delta=1e-6)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for n in range(ITERS):
            r.iterate(n)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    out = r.finish()  # the one read
    console.check_parameters()
    history, report = out[7]["loss"], out[8]
    assert len(history) == ITERS and report.iterations_run == ITERS
    assert (report.best_iteration, report.best_loss, report.settled_at) == tuple(R.replay(history, 1e-6, 3)[i] for i in (0, 1, 3))
    assert report.best_iteration > 0 and report.best_loss < history[0]  # and the loop did its work


# ---- optimize_batch(keep_best=True, patience=...) ----------------------------------------------------------------------------------
def batch_fit(bump, n_iters, callback=None, **kw):
    import test_online_batch_gpu as TB
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_batch

    tracks, ref = TB.songs((0, 1, 2))
    console, loss = AdvancedMixConsole(44100), Bumped(AudioFeatureLoss(G.WEIGHTS, 44100), bump.to(DEV))
    torch.manual_seed(0)
    out = optimize_batch(tracks, ref, console, loss, n_iters=n_iters, lr=LR, callback=callback, keep_best=True, **kw)
    return out, console, loss, tracks


class CaptureAndPoison:
    """The logits of every iteration, and a NaN into item 1's track gradient at one iteration."""

    def __init__(self, at):
        self.at, self.logits = at, []

    def __call__(self, n, view):
        self.logits.append([t.clone() for t in view.logits])
        if n == self.at:
            view.grads[0][1, 1, 3] = float("nan")


def test_batch_reports_pick_and_best_of():
    import test_online_gpu as G
    from mst.online import best_of, pick, render_blocks

    n_iters, patience, poisoned = 12, 4, 3
    bump = torch.zeros(n_iters, 3)
    bump[6:, 2] = BIG  # item 2 cannot improve from iteration 6 on: it settles at 9 at the latest
    bump[-2:, :2] = BIG  # the others do not end on their best
    cap = CaptureAndPoison(poisoned)
    out, console, loss, tracks = batch_fit(bump, n_iters, callback=cap, patience=patience)
    assert len(out) == 10 and out[8] == [None, poisoned, None]  # stopped_at as ever
    history, report = out[7]["loss"], out[9]
    assert tuple(history.shape) == (n_iters, 3) and report.iterations_run == [n_iters] * 3
    for b in range(3):
        at, best, _, settled = R.replay(history[:, b].tolist(), 0.0, patience, skip=(poisoned,) if b == 1 else ())
        print(f"[batch item {b}] best iteration {report.best_iteration[b]} loss {report.best_loss[b]:.6e} settled at {report.settled_at[b]}")
        assert (report.best_iteration[b], report.best_loss[b], report.settled_at[b]) == (at, best, settled)
        assert at < n_iters - 1
        for got, seen in zip((out[1], out[3], out[5]), cap.logits[at]):
            assert G.same_bits(got[b], seen[b])
        assert torch.equal(out[0][b], loss.mixes[at][b])
    assert report.settled_at[2] is not None and report.settled_at[2] <= 9
    assert report.best_iteration[1] is not None  # the item that met a NaN reports the best of its finite iterations
    winner = min(range(3), key=lambda b: report.best_loss[b])
    top = best_of(out)
    assert len(top) == 8 and G.same_bits(top[0], out[0][winner]) and G.same_bits(top[1], out[1][winner:winner + 1])
    for one, b in ((top, winner), (pick(out, 2), 2)):
        assert [tuple(one[i].shape) for i in (0, 1, 3, 5)] == [(2, 32768), (1, 3, 27), (1, 25), (1, 26)]
        full = render_blocks(tracks[b], *one[1:6:2], console, block_size=32768)  # one block: the best fit's mix, at batch 1
        print(f"[batch item {b}] render_blocks against the returned mix: max |difference| {float((full - out[0][b]).abs().max()):.3e}")
        assert tuple(full.shape) == (2, 32768) and bool(torch.isfinite(full).all()) and bool(full.any())


def test_poll_every_leaves_the_loop_when_every_item_has_settled():
    n_iters, patience = ITERS, 2
    bump = torch.zeros(n_iters, 3)
    bump[:3] = torch.tensor([3.0e4, 2.0e4, 1.0e4]).view(3, 1)  # steps far above what the fit itself moves: iterations 1 and 2 improve,
    bump[3:] = BIG  # nothing does from iteration 3 on: the wait is 1 at iteration 3 and every item settles at iteration 4
    out, _, loss, _ = batch_fit(bump, n_iters, patience=patience, poll_every=2)
    history, report = out[7]["loss"], out[9]
    ran = report.iterations_run[0]
    assert report.iterations_run == [ran] * 3 and ran == 6 < n_iters  # the poll after iteration 5 is the first to see all settled
    assert tuple(history.shape) == (ran, 3) and len(loss.mixes) == ran and out[8] == [None] * 3
    for b in range(3):
        at, best, _, settled = R.replay(history[:, b].tolist(), 0.0, patience)
        assert (report.best_iteration[b], report.best_loss[b], report.settled_at[b]) == (at, best, settled)
        assert (at, settled) == (2, 4)


def test_every_item_without_a_finite_iteration_raises():
    class PoisonAll:
        def __call__(self, n, view):
            view.grads[0][:, 1, 3] = float("nan")

    with pytest.raises(FloatingPointError, match="no iteration"):
        batch_fit(torch.zeros(2, 3), 2, callback=PoisonAll())


def test_errors():
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize, optimize_batch

    tracks, ref = G.song(0)
    console, loss = AdvancedMixConsole(44100), AudioFeatureLoss(G.WEIGHTS, 44100)
    for kw in (dict(patience=3), dict(keep_best=True, poll_every=2), dict(keep_best=True, min_delta=-1.0),
               dict(keep_best=True, patience=-2)):
        with pytest.raises(ValueError):
            optimize(tracks, ref, console, loss, n_iters=1, **kw)
        with pytest.raises(ValueError):
            optimize_batch(tracks, ref, console, loss, n_iters=1, batch=2, **kw)
