"""Batched and sectioned fits on the per-item MR-STFT loss (``MultiResolutionSTFTLoss.per_item`` / ``pooled``), end to end on the
MI355X: ``optimize_batch`` against a paired reference, ``optimize_sections``, ``optimize_sections_batch``, ``keep_best``, and a batch
of one beside ``optimize``.  T = 3 tracks of 16384 samples (the songs of tests/test_online_gpu.py), the reference's three resolutions,
a console with ``validate="deferred"``, 4 iterations.  Every run is replayed from a capturing callback: the history's loss column is the
loss evaluated again on the captured parameters' mix, bit for bit, and every item's logits after every step are those of the pinned
single-fit step (``mst_logit_adam_step``, tests/online_ref.py) fed the captured gradients, an item's section rows summed in section
order on the host."""
import functools

import pytest
import torch

import online_ref as O
import online_sections_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, N, ITERS, LR = 3, 16384, 4, 1e-3


@pytest.fixture()
def drv():
    from mst import _hip

    d = O.Driver(_hip.lib(), DEV)
    yield d
    from online_batch_ref import scrub

    scrub(d)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(O.bits(a), O.bits(b))


def make_loss():
    from mst.loss import MultiResolutionSTFTLoss

    return MultiResolutionSTFTLoss(fft_sizes=[512, 2048, 8192], hop_sizes=[256, 1024, 4096], win_lengths=[512, 2048, 8192])


def song(seed, n=N):
    import test_online_gpu as G

    return G.song(seed, T, n)


def fit(fn, tracks, ref, seed=0, n_iters=ITERS, **kw):
    import test_online_gpu as G
    from mst.modules import AdvancedMixConsole

    console, cap, loss = AdvancedMixConsole(44100, validate="deferred"), G.Capture(), make_loss()
    torch.manual_seed(seed)
    out = fn(tracks, ref, console, loss, n_iters=n_iters, lr=LR, callback=cap, **kw)
    console.check_parameters()
    return out, cap, console, loss


def check_replay(drv, out, cap, items, sections, history):
    """Every item through a single-fit session of the pinned step: its captured gradient rows summed in section order, its captured
    loss as the one term -> its logits after every step and its history column, bit for bit."""
    assert [g is None for g in cap.grads[0]] == [False, True, False]  # use_fx_bus=False: the fx parameters have no gradient
    n_iters = len(cap.grads)
    for b in range(items):
        theta0 = [t[b].cpu().reshape(-1) for t in cap.logits[0]]
        ses = O.Session(drv, theta0, n_iters, 1)
        for k in range(n_iters):
            grads = [None if g is None else P.host_sum(g.cpu().reshape(items, sections, -1)[b]).to(DEV) for g in cap.grads[k]]
            ses.step(grads, cap.losses[k].reshape(items)[b:b + 1].clone(), LR)
            after = cap.logits[k + 1] if k + 1 < n_iters else (out[1], out[3], out[5])
            for got, want in zip(after, ses.theta):
                assert same_bits(got[b].reshape(-1), want), f"item {b}: the logits after step {k} differ from the replayed session's"
        assert torch.equal(O.bits(history[:, b]), O.bits(ses.history.cpu()[:, 0]))
    drv.check_guards()


def check_history_is_the_loss_again(out_history, cap, console, tracks_rows, evaluate):
    """history[k] is the loss of the mix of iteration k's captured parameters, evaluated again (the value-only route), bit for bit"""
    for k, params in enumerate(cap.params):
        with torch.no_grad():
            mix = console(tracks_rows, *params, use_fx_bus=False)[1]
            again = evaluate(mix)
        assert same_bits(cap.losses[k].detach().reshape(-1), again.reshape(-1)), k
        assert torch.equal(O.bits(out_history[k].reshape(-1)), O.bits(again.cpu().reshape(-1))), k
    assert bool(torch.isfinite(out_history).all())


def test_a_batch_against_one_paired_reference(drv):
    from mst.online import optimize_batch

    tracks, ref = song(0)
    out, cap, console, loss = fit(optimize_batch, tracks, ref, batch=3)
    assert len(out) == 9 and out[8] == [None] * 3 and list(out[7]) == ["loss"]
    assert [tuple(t.shape) for t in (out[0], out[1], out[3], out[5])] == [(3, 2, N), (3, T, 27), (3, 25), (3, 26)]
    history = out[7]["loss"]
    assert tuple(history.shape) == (ITERS, 3) and len({float(v) for v in history[0]}) == 3  # three start points
    rows = tracks[None].repeat(3, 1, 1)
    check_history_is_the_loss_again(history, cap, console, rows, lambda mix: loss.per_item(mix, ref[None].expand(3, -1, -1)))
    check_replay(drv, out, cap, 3, 1, history)
    # (2, n) against (B, T, n) reached the kernels as B dense rows: the loop's first value is per_item on a materialised copy
    with torch.no_grad():
        mix = console(rows, *cap.params[0], use_fx_bus=False)[1]
        dense = loss.per_item(mix, ref[None].repeat(3, 1, 1))
    assert same_bits(dense.cpu(), history[0])


def sections_of(seed):
    from mst.online import take_sections

    tracks, ref = song(seed, 2 * N)
    cut, ref_cut = take_sections(tracks, (0, N), N), take_sections(ref, (0, N), N)
    assert tuple(cut.shape) == (2, T, N) and tuple(ref_cut.shape) == (2, 2, N)
    return cut, ref_cut


def test_two_sections_of_one_fit(drv):
    from mst.online import optimize_sections

    cut, ref_cut = sections_of(0)
    out, cap, console, loss = fit(optimize_sections, cut, ref_cut)
    assert len(out) == 8 and list(out[7]) == ["loss"] and len(out[7]["loss"]) == ITERS
    assert [tuple(t.shape) for t in (out[0], out[1], out[3], out[5])] == [(2, 2, N), (1, T, 27), (1, 25), (1, 26)]
    assert tuple(cap.losses[0].shape) == (1,) and [tuple(g.shape) for g in (cap.grads[0][0], cap.grads[0][2])] == [(2, T, 27), (2, 26)]
    history = torch.tensor(out[7]["loss"])[:, None]
    check_history_is_the_loss_again(history, cap, console, cut, lambda mix: loss.pooled(mix, ref_cut))
    check_replay(drv, out, cap, 1, 2, history)
    # pooling is the loss of the sections taken as one batch
    with torch.no_grad():
        mix = console(cut, *cap.params[0], use_fx_bus=False)[1]
        assert same_bits(loss(mix, ref_cut).reshape(1).cpu(), history[0])


def test_two_items_of_two_sections(drv):
    from mst.online import optimize_sections_batch

    (cut0, ref0), (cut1, ref1) = sections_of(0), sections_of(1)
    sections, refs = torch.stack((cut0, cut1)), torch.stack((ref0, ref1))
    out, cap, console, loss = fit(optimize_sections_batch, sections, refs)
    assert len(out) == 9 and out[8] == [None, None] and list(out[7]) == ["loss"]
    assert [tuple(t.shape) for t in (out[0], out[1], out[3], out[5])] == [(2, 2, 2, N), (2, T, 27), (2, 25), (2, 26)]
    history = out[7]["loss"]
    rows, ref_rows = sections.reshape(4, T, N), refs.reshape(4, 2, N)
    check_history_is_the_loss_again(history, cap, console, rows, lambda mix: loss.pooled(mix, ref_rows, items=2))
    check_replay(drv, out, cap, 2, 2, history)
    # one (S, 2, n) reference serves every item: restarts of item 0 see what item 0 saw
    shared, cap2, _, _ = fit(optimize_sections_batch, cut0, ref0, batch=2)
    assert same_bits(shared[7]["loss"][:, 0], history[:, 0])
    assert not same_bits(shared[7]["loss"][:, 1], history[:, 1])


def test_keep_best_reports_every_items_minimum():
    from mst.online import FitReport, best_of, optimize_batch

    tracks, ref = song(0)
    out, _, _, _ = fit(optimize_batch, tracks, ref, batch=3, n_iters=6, keep_best=True)
    assert len(out) == 10 and isinstance(out[9], FitReport)
    history = out[7]["loss"]
    for b in range(3):
        assert out[9].best_loss[b] == float(history[:, b].min())
        assert out[9].best_iteration[b] == int(history[:, b].argmin())
    picked = best_of(out)
    assert min(picked[7]["loss"]) == min(out[9].best_loss)


def test_a_batch_of_one_beside_optimize():
    import test_online_gpu as G
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize, optimize_batch

    tracks, ref = song(0)
    out, cap, _, _ = fit(optimize_batch, tracks[None], ref[None])
    single_cap = G.Capture()
    torch.manual_seed(0)
    single = optimize(tracks, ref, AdvancedMixConsole(44100, validate="deferred"), make_loss(), n_iters=ITERS, lr=LR, callback=single_cap)
    for a, b in zip(cap.logits[0], single_cap.logits[0]):
        assert same_bits(a, b)  # the same start point
    assert list(single[7]) == ["loss"]
    # the first history row bit for bit: one item of two rows is the batch loss of those rows (no 1 / items to differ by)
    assert float(out[7]["loss"][0, 0]) == single[7]["loss"][0]
    assert same_bits(cap.losses[0].reshape(()), single_cap.losses[0].reshape(()))
    for g, h in zip(cap.grads[0], single_cap.grads[0]):
        assert (g is None) == (h is None) and (g is None or same_bits(g, h))
