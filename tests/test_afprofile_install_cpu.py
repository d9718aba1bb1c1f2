"""Feature profiles through ``diffmst_hip.install()`` against the REAL reference package (build container only: needs
/root/reference), in the pattern of tests/test_install_cpu.py: the rebinding table is unchanged (five symbols), so after ``install()``
the new surface is reached through the rebound class - ``mst.loss.AudioFeatureLoss.Profile`` and ``.profile`` - and a profile target
must arrive at OUR loss, which refuses host tensors.  Runs in a subprocess: the reference's ``mst`` package must not meet the alias
package the rest of the suite imports.  The alias route (``from mst.loss import AudioFeatureProfile``) needs no reference."""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"

SCRIPT = textwrap.dedent(
    """
    import sys
    sys.dont_write_bytecode = True
    sys.path[:0] = [{root!r}, {root!r} + "/tests"]
    import refstubs
    refstubs.install_stubs()
    sys.path.insert(0, {ref!r})                       # the reference checkout, as a user has it
    sys.path.append({root!r} + "/diff-mst_amd")       # diffmst_hip only - NOT diff-mst_amd/standalone
    import torch
    import mst.loss                                   # the reference's own module
    assert set(mst.__path__) == {{{ref!r} + "/mst"}}, list(mst.__path__)
    ref_cls = mst.loss.AudioFeatureLoss
    assert not hasattr(ref_cls, "Profile") and not hasattr(ref_cls, "profile")
    import diffmst_hip
    assert len(diffmst_hip.install()) == 5
    assert mst.loss.AudioFeatureLoss is diffmst_hip.loss.AudioFeatureLoss
    assert mst.loss.AudioFeatureLoss.Profile is diffmst_hip.loss.AudioFeatureProfile
    # a stored profile reloads through the rebound name; its views are host arithmetic on the 54 numbers
    d = torch.zeros(1, 54, dtype=torch.float64)
    d[0, :6] = torch.tensor([0.04, 0.01, 0.09, 0.01, 0.4, 0.2])
    p = mst.loss.AudioFeatureLoss.Profile(d, 44100)
    assert torch.allclose(p.rms, torch.tensor([[0.2, 0.1]])) and tuple(p.barkspectrum.shape) == (1, 24, 2)
    f = mst.loss.AudioFeatureLoss([0.1, 0.001, 1.0, 1.0, 0.1], 44100)
    x = torch.zeros(1, 2, 20000)
    for call in (lambda: f(x, p), lambda: f(x, torch.zeros(1, 2, 33000)), lambda: f.profile(x)):
        try:
            call()
        except RuntimeError as e:                     # OUR loss, reached through the reference's name: it has no host path
            assert "CPU tensor" in str(e), e
        else:
            raise AssertionError("a host tensor was accepted")
    try:
        f(x, p.sample_rate)
    except TypeError as e:
        assert "AudioFeatureProfile" in str(e), e
    else:
        raise AssertionError("an int was accepted as target")
    diffmst_hip.uninstall()
    assert mst.loss.AudioFeatureLoss is ref_cls
    print("PROFILE_AFTER_INSTALL_OK")
    """
)


# Not self-contained by design, like tests/test_install_cpu.py: its subject is the reference package itself.  It runs where a checkout
# of the reference is readable and skips elsewhere; the alias-package case below needs none.
@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference checkout (build container only)")
def test_profile_is_reachable_through_mst_loss_after_install():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-B", "-c", SCRIPT.format(root=ROOT, ref=REF)], capture_output=True, text=True, env=env,
                       cwd="/tmp", timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PROFILE_AFTER_INSTALL_OK" in r.stdout, r.stdout + r.stderr


def test_profile_is_exported_by_the_alias_package():
    import diffmst_hip.loss
    import mst.loss

    assert mst.loss.AudioFeatureProfile is diffmst_hip.loss.AudioFeatureProfile is mst.loss.AudioFeatureLoss.Profile
    assert callable(mst.loss.AudioFeatureLoss.profile)
