"""Linked rows on the MI355X: the cases of tests/test_online_links_hostsim.py (tests/online_links_ref.py) on the product library at 50
steps, then ``mst.online.optimize`` / ``optimize_sections_batch`` with ``stereo_id`` / ``links`` end to end: the captured gradients of
every iteration replayed through ``LinkedSession``s bit for bit, plain and with ``keep_best``, the invariants of the returned logits and
the mirrored pan of the returned dictionary.  T = 4, n = 17000, a reference of 20000 samples."""
import functools

import pytest
import torch

import online_links_ref as K
import online_ref as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, N, M, ITERS, LR = 4, 17000, 20000, 5, 1e-3
STEREO_ID = [1, 0, 0, 0]
LEADERS = [0, 0, 2, 3]


@pytest.fixture()
def drv():
    from mst import _hip

    d = O.Driver(_hip.lib(), DEV)
    yield d
    from online_batch_ref import scrub

    scrub(d)


# ---- the step through the C ABI: the simulator's cases at 50 steps -----------------------------------------------------------------------
@pytest.mark.parametrize("best", [False, True])
@pytest.mark.parametrize("rows", [3, 10])
@pytest.mark.parametrize("items,sections", [(1, 1), (2, 2), (3, 3)])
def test_identity_map_is_the_sections_batch_call(drv, items, sections, rows, best):
    K.check_identity_is_sections_batch(drv, items, sections, rows, best)


@pytest.mark.parametrize("sections", [1, 3])
@pytest.mark.parametrize("name", sorted(K.MAPS))
def test_linked_step_matches_adam_on_the_leader_rows(drv, name, sections, record):
    K.check_parity(drv, name, sections, 50, record)


def test_zero_logits_pan_both_channels_to_the_centre(drv):
    K.check_zero_logits_pan_centre(drv)


@pytest.mark.parametrize("where", ["nan", "overflow"])
def test_nonfinite_follower_or_group_sum_stops_its_item_alone(drv, where):
    K.check_nonfinite_follower(drv, where)


@pytest.mark.parametrize("which", [0, 1])
def test_null_gradient_segment_keeps_its_bits(drv, which):
    K.check_null_gradient(drv, which)


def test_best_snapshot_is_the_iterate_before_the_update_for_every_member(drv):
    K.check_best_snapshot(drv)


@pytest.mark.parametrize("best", [False, True])
def test_every_item_is_a_single_item_linked_session(drv, best):
    K.check_items_are_single_sessions(drv, best)


def test_unsupported_arguments_launch_nothing(drv):
    K.check_refusals(drv)


# ---- optimize() with links end to end ----------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and torch.equal(O.bits(a), O.bits(b))


@functools.lru_cache(maxsize=None)
def material(seed):
    """(tracks (T, 2 N), reference mix (2, M)) on the device: tests/test_online_gpu.py's coloured noise and console-made reference."""
    import test_online_gpu as G

    return G.coloured_tracks(T, 2 * N, seed).to(DEV), G.song(seed, T, M)[1]


def fit_single(**kw):
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize

    tracks, ref = material(0)
    cap = G.Capture()
    torch.manual_seed(0)
    out = optimize(tracks[:, :N].contiguous(), ref, AdvancedMixConsole(44100), AudioFeatureLoss(G.WEIGHTS, 44100), n_iters=ITERS, lr=LR,
                   callback=cap, **kw)
    return out, cap


@functools.lru_cache(maxsize=None)
def linked_single(keep_best):
    """One captured linked fit, shared by the cases below and never modified."""
    return fit_single(stereo_id=STEREO_ID, **(dict(keep_best=True) if keep_best else {}))


def replay(drv, cap, items, sections, best):
    """The captured gradients and loss terms of every iteration through a ``LinkedSession`` that starts at the captured logits."""
    keys = list(cap.losses[0])
    theta0 = [[t[b].cpu().reshape(-1) for t in cap.logits[0]] for b in range(items)]
    ses = K.LinkedSession(drv, theta0, sections, len(cap.grads), len(keys), K.make_links(LEADERS), best=best)
    for k in range(len(cap.grads)):
        grads = [None if g is None else g.reshape(items, sections, -1).contiguous() for g in cap.grads[k]]
        terms = torch.stack([cap.losses[k][name].reshape(items) for name in keys], dim=1).contiguous()
        ses.step(grads, terms, LR)
    return ses, keys


def assert_linked(logits, tag):
    rows = logits.reshape(-1, T, K.COLS)
    flip = O.bits(K.sign_of(LEADERS).float()) & K.SIGN_BIT
    for th in rows.cpu():
        assert torch.equal(O.bits(th), O.bits(th[torch.tensor(LEADERS)]) ^ flip), f"{tag}: a follower's logits are not its leader's"
        assert not same_bits(th[2], th[3]) and not same_bits(th[0], th[2]), f"{tag}: unlinked rows came out equal"


def assert_mirrored_pan(track_dict, tag):
    pan = track_dict["stereo_panner"]["pan"].detach().cpu().reshape(-1, T)
    ulp = 2.0 ** -23  # of 1: what online_ref.SIGMOID_MARGIN_ULP grants a second exp
    worst = float((pan[:, 1].double() - (1.0 - pan[:, 0].double())).abs().max())
    print(f"\n[{tag}] pan_l = {pan[:, 0].tolist()}, pan_f = {pan[:, 1].tolist()}, |pan_f - (1 - pan_l)| = {worst:.3e}")
    assert worst <= O.SIGMOID_MARGIN_ULP * ulp


def test_linked_optimize_replays_through_a_linked_session(drv):
    out, cap = linked_single(False)
    assert [g is None for g in cap.grads[0]] == [False, True, False]
    assert_linked(cap.logits[0][0], "the start point")  # the init launch overwrote the followers
    from mst.modules import AdvancedMixConsole
    from mst.online import start_point

    torch.manual_seed(0)
    drawn = start_point(T, AdvancedMixConsole(44100), 0.001)  # all T rows are drawn: the leaders and the free rows keep the script's
    assert same_bits(cap.logits[0][0][0, [0, 2, 3]].cpu(), drawn[0][[0, 2, 3]]) and same_bits(cap.logits[0][2].cpu(), drawn[2])
    ses, keys = replay(drv, cap, 1, 1, False)
    for got, want in zip((out[1], out[3], out[5]), ses.theta):
        assert same_bits(got.reshape(-1), want), "the logits differ from the replayed session's"
    history = ses.history.cpu()[:, 0]
    assert out[7]["loss"] == history[:, 0].tolist() and all(out[7][name] == history[:, 1 + j].tolist() for j, name in enumerate(keys))
    for params in cap.params:  # the p the console consumed: the session's invariants on the live tensors
        p = params[0][0].cpu()
        assert same_bits(p[1, :K.PAN], p[0, :K.PAN]) and same_bits(p[1, K.PAN + 1:], p[0, K.PAN + 1:])
    assert_linked(out[1], "the returned logits")
    assert_mirrored_pan(out[2], "optimize, stereo_id")
    K.assert_invariants(drv, ses, LEADERS, "replay")


def test_linked_optimize_with_keep_best_returns_the_best_members(drv):
    from mst import online

    out, cap = linked_single(True)
    assert len(out) == 9 and isinstance(out[8], online.FitReport)
    ses, _ = replay(drv, cap, 1, 1, True)
    block = ses.best[0].cpu()
    assert block[0].item() == out[8].best_iteration + 1
    stored = block[K.B.BEST_HDR:K.B.BEST_HDR + ses.n].view(torch.float32)
    assert same_bits(torch.cat([t.reshape(-1) for t in (out[1], out[3], out[5])]).cpu(), stored)
    assert same_bits(out[1].cpu(), cap.logits[out[8].best_iteration][0].cpu())  # the iterate the best loss was evaluated at
    assert_linked(out[1], "the best logits")
    assert_mirrored_pan(out[2], "optimize, keep_best")
    plain, _ = linked_single(False)
    assert out[7] == plain[7]  # the same run


def test_links_and_stereo_id_say_the_same_and_unlinked_rows_are_free():
    a, _ = linked_single(False)
    b, _ = fit_single(links=LEADERS)
    assert all(same_bits(a[i], b[i]) for i in (0, 1, 3, 5)) and a[7] == b[7]
    free, _ = fit_single()
    th = free[1][0].cpu()
    assert not same_bits(th[1], th[0])  # what the feature is for: without links the two halves of the pair drift apart


def test_linked_sections_batch_replays_through_a_linked_session(drv):
    import test_online_gpu as G
    from mst.loss import AudioFeatureLoss
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize_sections_batch, pick, take_sections

    sections = torch.stack([take_sections(material(s)[0], (0, N), N) for s in (0, 1)])  # (2, 2, T, N)
    refs = torch.stack([material(s)[1] for s in (0, 1)])
    cap = G.Capture()
    torch.manual_seed(0)
    out = optimize_sections_batch(sections, refs, AdvancedMixConsole(44100), AudioFeatureLoss(G.WEIGHTS, 44100), n_iters=ITERS, lr=LR,
                                  callback=cap, stereo_id=STEREO_ID)
    assert [tuple(t.shape) for t in (out[0], out[1], out[3], out[5])] == [(2, 2, 2, N), (2, T, 27), (2, 25), (2, 26)] and out[8] == [None, None]
    ses, keys = replay(drv, cap, 2, 2, False)
    for got, want in zip((out[1], out[3], out[5]), ses.theta):
        assert same_bits(got.reshape(-1), want), "the logits differ from the replayed session's"
    history = ses.history.cpu()
    assert torch.equal(O.bits(out[7]["loss"]), O.bits(history[:, :, 0]))
    for params in cap.params:  # rows b S + s: equal within an item, linked within a row
        assert same_bits(params[0][0], params[0][1]) and same_bits(params[0][2], params[0][3]) and not same_bits(params[0][0], params[0][2])
    assert_linked(out[1], "the returned logits")
    assert not same_bits(out[1][0], out[1][1])
    assert_mirrored_pan(out[2], "optimize_sections_batch, stereo_id")
    assert_mirrored_pan(pick(out, 1)[2], "pick(1)")
    K.assert_invariants(drv, ses, LEADERS, "replay")
