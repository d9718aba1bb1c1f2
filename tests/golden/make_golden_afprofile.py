#!/usr/bin/env python3
"""Generate tests/golden/af_loss_unequal.npz FROM THE REAL REFERENCE: ``AudioFeatureLoss`` on an input and a target of different
lengths (mst/loss.py:127-260 reduce every feature over time, so the class takes them; scripts/online.py relies on it).

Works as make_golden.py does - same stubs, same location of the reference, build container only:
    python -B tests/golden/make_golden_afprofile.py
Imports the reference's own ``mst.loss``, asserts that the oracle's restatement reproduces its five losses at rtol 1e-6 and writes
input (2, 2, 20000), target (2, 2, 33000), the weights, the losses, and a 1-in-16 subsample and the L2 norm of the input gradient
of ``sum(v.mean() for v in losses.values())`` (mst/system.py:334-336).  The fixture is data; no reference source is stored.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg
from oracle import loss_restated as ol


def main():
    assert os.path.isdir(mg.REF), "golden generation needs the reference checkout (build container only)"
    mg.install_stubs()
    sys.path.insert(0, mg.REF)
    import mst.loss as rloss

    weights = [0.1, 0.001, 1.0, 1.0, 0.1]  # unpaired+feat.yaml:55-60
    torch.manual_seed(23)
    a = (0.2 * torch.randn(2, 2, 20000)).requires_grad_(True)
    b = 0.3 * torch.randn(2, 2, 33000) * torch.tensor([1.0, 0.6]).view(1, 2, 1)
    ld = rloss.AudioFeatureLoss(weights=weights, sample_rate=44100)(a, b)
    sum(v.mean() for v in ld.values()).backward()
    old = ol.audio_feature_loss(a.detach(), b, weights)
    assert list(ld.keys()) == list(ol.AF_KEYS)
    for k in ld:
        assert torch.allclose(ld[k].detach(), old[k], rtol=1e-6, atol=0), k
    out = os.path.join(HERE, "af_loss_unequal.npz")
    np.savez_compressed(
        out, input=a.detach().numpy(), target=b.numpy(), weights=np.array(weights),
        grad_input_sub=a.grad.numpy()[..., ::16], grad_input_l2=np.array(a.grad.pow(2).sum().sqrt().item()),
        **{"loss." + k: v.detach().numpy() for k, v in ld.items()},
    )
    print(out, os.path.getsize(out), "bytes;", {k: v.item() for k, v in ld.items()})


if __name__ == "__main__":
    main()
