"""Feature profiles of AudioFeatureLoss (diff-mst_amd/csrc/mst_af.hip, ABI v13) on the host simulator, through the C ABI: a target of
another length analysed once into 54 numbers, the loss and its backward against them.  Three frames per signal - the smallest shapes at
which the strip plan, the reflected edge frames and the ragged rows all occur - and the two fixtures the reference's own class wrote
(tests/golden/af_loss.npz, af_loss_unequal.npz: three to five frames); tests/test_afprofile_gpu.py carries the same cases
(tests/afprofile_ref.py) at the reference's sizes on the device."""
import pytest
import torch

import afprofile_ref as R


@pytest.fixture(scope="module")
def drv():
    from hostsim import harness

    return R.Driver(harness.lib(), "cpu")


@pytest.mark.parametrize("bs,n_pred,n_target", [(1, 17000, 16400), (2, 17000, 20000)])
def test_unequal_lengths_three_way(drv, bs, n_pred, n_target, record):
    R.check_three_way(drv, bs, n_pred, n_target, record)


def test_profile_views_against_the_reference_functions(drv, record):
    R.check_golden_features(drv, record)


@pytest.mark.parametrize("fixture", ["af_loss.npz", "af_loss_unequal.npz"])
def test_loss_against_the_reference_class(drv, fixture, record):
    R.check_golden_loss(drv, fixture, record)


def test_known_answers(drv):
    R.check_known_answers(drv, bs=1, n=16390)


def test_determinism_and_bounds_of_writes(drv):
    R.check_determinism_and_bounds(drv, 1, 16387, 16403)


def test_validation(drv):
    R.check_validation(drv)


def test_profile_views_on_the_host():
    """The views are torch operations on the 54 numbers: units, shapes and clamps of the reference's compute_* functions."""
    from mst.loss import AudioFeatureProfile

    d = torch.zeros(2, 54, dtype=torch.float64)
    d[0, :6] = torch.tensor([0.04, 0.01, 0.09, 0.01, 0.4, 0.2])
    d[:, 6:30], d[:, 30:] = 1.5, -2.5
    p = AudioFeatureProfile(d, 44100)
    assert p.batch_size == 2 and p.n_samples is None and p.sample_rate == 44100
    assert torch.allclose(p.rms, torch.tensor([[0.2, 0.1], [1e-4, 1e-4]]))  # sqrt(clamp(mean square, 1e-8))
    assert torch.allclose(p.crest_factor[0], torch.tensor([6.0206, 6.0206]), atol=1e-4) and bool(((p.crest_factor[1] + 160.0).abs() < 1e-4).all())
    assert torch.allclose(p.stereo_width, torch.tensor([1.0 / 9.0, 0.0])) and torch.allclose(p.stereo_imbalance, torch.tensor([-0.6, 0.0]))
    assert tuple(p.barkspectrum.shape) == (2, 24, 2) and bool((p.barkspectrum[..., 0] == 1.5).all()) and bool((p.barkspectrum[..., 1] == -2.5).all())
    assert all(getattr(p, name).dtype == torch.float32 and not getattr(p, name).requires_grad for name, _ in R.FEATS)
    assert p.to("cpu").data.data_ptr() == p.data.data_ptr() and p.to("cpu").sample_rate == 44100
    for bad in (torch.zeros(2, 53, dtype=torch.float64), torch.zeros(2, 54), torch.zeros(54, dtype=torch.float64)):
        with pytest.raises(ValueError):
            AudioFeatureProfile(bad, 44100)


def test_a_target_that_is_neither_tensor_nor_profile_is_a_type_error():
    from mst.loss import AudioFeatureLoss
    from mst.online import optimize

    f, x = AudioFeatureLoss(R.AF_WEIGHTS, 44100), torch.zeros(1, 2, 20000)
    for target in (None, x.numpy(), [0.0] * 54):
        with pytest.raises(TypeError, match="AudioFeatureProfile"):
            f(x, target)
    with pytest.raises(TypeError, match="AudioFeatureProfile"):
        optimize(x[0], x[0].numpy(), None, f)
