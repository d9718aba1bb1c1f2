"""The best-iterate keywords of ``mst.online.optimize`` / ``optimize_batch``, ``pick`` and ``best_of`` without a GPU: what is wrong with
a call is said before anything touches a device, and the two selectors work on host tuples."""
import pytest
import torch


class PerItem:
    def per_item(self, mix, target):
        raise AssertionError("the loss was called")


def test_alias_exports_and_signatures():
    import diffmst_hip
    import mst.online
    from mst import _cabi

    assert mst.online is diffmst_hip.online
    for name in ("best_of", "pick", "optimize", "optimize_batch"):
        assert callable(getattr(mst.online, name))
    assert mst.online.FitReport._fields == ("best_iteration", "best_loss", "settled_at", "iterations_run")
    for name in ("mst_logit_adam_best_bytes", "mst_logit_adam_step_best", "mst_logit_adam_step_best_batch"):
        assert name in _cabi.SIGNATURES


BAD = (
    (dict(patience=3), "keep_best"),
    (dict(keep_best=True, poll_every=2), "patience"),
    (dict(poll_every=2), "patience"),
    (dict(keep_best=True, patience=-1), "patience"),
    (dict(keep_best=True, patience=2.5), "patience"),
    (dict(keep_best=True, min_delta=-0.5), "min_delta"),
    (dict(keep_best=True, min_delta=float("nan")), "min_delta"),
    (dict(keep_best=True, min_delta=float("inf")), "min_delta"),
    (dict(keep_best=True, min_delta=1e39), "min_delta"),
    (dict(min_delta=0.5), "keep_best"),
    (dict(keep_best=True, patience=2, poll_every=0), "poll_every"),
)


@pytest.mark.parametrize("kw, match", BAD)
def test_keyword_errors_come_before_any_device_call(kw, match):
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize, optimize_batch

    console = AdvancedMixConsole(44100)
    with pytest.raises(ValueError, match=match):
        optimize(torch.zeros(2, 32768), torch.zeros(2, 32768), console, lambda a, b: None, **kw)
    with pytest.raises(ValueError, match=match):
        optimize_batch(torch.zeros(3, 2, 32768), torch.zeros(3, 2, 32768), console, PerItem(), **kw)


def test_well_formed_keywords_get_as_far_as_the_device_check():
    from mst.modules import AdvancedMixConsole
    from mst.online import optimize

    with pytest.raises(RuntimeError, match="CPU tensor"):
        optimize(torch.zeros(2, 32768), torch.zeros(2, 32768), AdvancedMixConsole(44100), lambda a, b: None, n_iters=1, keep_best=True,
                 patience=3, min_delta=0.25, poll_every=2)


def batch_result(with_report):
    from mst.online import FitReport

    B, T, N = 3, 2, 8
    dicts = [{"fx": {"gain": torch.arange(float(B * k)).reshape(B, k)}} for k in (T, 1, 1)]
    history = {"loss": torch.arange(12.0).reshape(4, B), "rms": torch.ones(4, B)}
    result = (torch.arange(float(B * 2 * N)).reshape(B, 2, N), torch.zeros(B, T, 27), dicts[0], torch.zeros(B, 25), dicts[1],
              torch.arange(float(B * 26)).reshape(B, 26), dicts[2], history, [None, 2, None])
    return result + ((FitReport([3, None, 1], [0.5, float("inf"), 0.25], [None, None, 3], [4, 4, 4]),) if with_report else ())


def test_pick_takes_the_longer_tuple():
    from mst.online import pick

    short, long = batch_result(False), batch_result(True)
    for b in (0, 1, -1):
        a, c = pick(short, b), pick(long, b)
        assert len(a) == len(c) == 8 and a[7] == c[7]
        for i in (0, 1, 3, 5):
            assert torch.equal(a[i], c[i])
    with pytest.raises(ValueError):
        pick(long + (None,), 0)
    with pytest.raises(IndexError):
        pick(long, 3)


def test_best_of_is_the_argmin_of_best_loss():
    from mst.online import FitReport, best_of, pick

    result = batch_result(True)
    got, want = best_of(result), pick(result, 2)
    assert len(got) == 8 and torch.equal(got[0], want[0]) and torch.equal(got[5], want[5]) and got[7] == want[7]
    tie = result[:9] + (FitReport([3, 0, 1], [0.25, 0.25, 0.25], [None] * 3, [4] * 3),)
    assert torch.equal(best_of(tie)[0], result[0][0])  # the first of equals
    with pytest.raises(ValueError):
        best_of(batch_result(False))
    with pytest.raises(ValueError):
        best_of(result[:9] + (FitReport([None] * 3, [float("inf")] * 3, [None] * 3, [4] * 3),))
