#!/usr/bin/env python3
"""Generate tests/golden/af_pooled.npz FROM THE REAL REFERENCE: the features of three sections of one signal taken together.

Works as make_golden_afprofile.py does - same stubs, same location of the reference, build container only:
    python -B tests/golden/make_golden_afpooled.py
Imports the reference's own ``mst.loss`` and records, for three sections (3, 2, 20000) scaled by 0.5, 1 and 1.5, its
``compute_rms``, ``compute_crest_factor``, ``compute_stereo_width`` and ``compute_stereo_imbalance`` of ``torch.cat(sections, dim=-1)``
and its ``compute_barkspectrum`` of every section, after asserting that the oracle's restatement reproduces each at rtol 1e-6.  The
fixture is data; no reference source is stored.
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

    torch.manual_seed(29)
    x = 0.2 * torch.randn(3, 2, 20000) * torch.tensor([0.5, 1.0, 1.5]).view(3, 1, 1)
    x[:, 1] = 0.6 * x[:, 1] + 0.3 * x[:, 0]
    whole = torch.cat(list(x), dim=-1).unsqueeze(0)  # (1, 2, 60000)
    out = dict(sections=x.numpy())
    for key, theirs, ours in (("rms", rloss.compute_rms, ol.feat_rms), ("crest", rloss.compute_crest_factor, ol.feat_crest_factor),
                              ("width", rloss.compute_stereo_width, ol.feat_stereo_width),
                              ("imbalance", rloss.compute_stereo_imbalance, ol.feat_stereo_imbalance)):
        got = theirs(whole)
        assert torch.allclose(got, ours(whole), rtol=1e-6, atol=0), key
        out["feat." + key] = got.numpy()
    bark = rloss.compute_barkspectrum(x, sample_rate=44100)  # (3, 24, 2): every section on its own
    assert torch.allclose(bark, ol.feat_barkspectrum(x), rtol=1e-6, atol=0)
    out["feat.bark_sections"] = bark.numpy()
    path = os.path.join(HERE, "af_pooled.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
