"""Generator of tests/golden/nmi.npz -- the reference's NMI_Loss (util/losses.py:263-348) on seeded inputs: the loss and
the gradients of BOTH arguments.  Runs only where the reference checkout (make_golden.REF) exists; imports the reference itself with the shims of
make_golden.py and records INPUTS-BY-SEED + the reference's own outputs, per case <tag>:

  <tag>_true, <tag>_pred, [<tag>_mask]   inputs (values below 0, above max_clip and exactly on both bounds included)
  <tag>_centers, <tag>_params            bin centers; [sigma_ratio, max_clip, crop_background]
  <tag>_loss, <tag>_dtrue, <tag>_dpred   -MI (shape (1,)) and its gradients

    python tests/golden/make_golden_nmi.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests.golden import common as C                      # noqa: E402
from tests.golden import make_golden as MG                # noqa: E402


def _image(seed, shape, max_clip):
    """Uniform on [-0.15, 1.15] * max_clip, with a few voxels exactly on 0 and on max_clip."""
    x = (C.rand(seed, *shape) * 1.3 - 0.15) * max_clip
    flat = x.view(-1)
    idx = (C.rand(seed + 1, 16) * flat.numel()).long()
    flat[idx[:8]] = 0.0
    flat[idx[8:]] = max_clip
    return x


def cases():
    """(tag, shape, centers, sigma_ratio, max_clip, mask or None)"""
    uni = lambda nb, top=1.0: np.linspace(0.0, top, nb)
    nonuni = (np.linspace(0.0, 1.0, 24) ** 1.6) * 1.5          # denser near 0, max_clip 1.5
    m3 = (C.rand(71, 1, 1, 10, 12, 14) > 0.35).float() * C.rand(72, 1, 1, 10, 12, 14)   # some values <= 1e-4
    m2 = (C.rand(73, 1, 1, 24, 20) > 0.4).float()               # [1,1,H,W] against B = 2
    return [
        ("2d_nb32", (2, 1, 24, 20), uni(32), 0.5, 1.0, None),
        ("3d_nb8", (1, 1, 10, 12, 14), uni(8), 0.5, 1.0, None),
        ("3d_nb32", (1, 1, 10, 12, 14), uni(32), 0.5, 1.0, None),
        ("3d_nb48", (1, 1, 10, 12, 14), uni(48), 0.7, 1.0, None),
        ("2d_nonuniform", (2, 1, 24, 20), nonuni, 0.5, 1.5, None),
        ("3d_crop_mask", (1, 1, 10, 12, 14), uni(32), 0.5, 1.0, m3),
        ("2d_crop_bcast", (2, 1, 24, 20), uni(32), 0.5, 1.0, m2),
    ]


def main():
    MG.install_shims()
    from util.losses import NMI_Loss as RefNMI
    npy = MG.npy
    out = {}
    for i, (tag, shape, centers, ratio, maxc, mask) in enumerate(cases()):
        yt = _image(100 + 10 * i, shape, maxc).requires_grad_()
        yp = _image(105 + 10 * i, shape, maxc)
        yp = (0.6 * yp + 0.4 * yt.detach()).requires_grad_()    # correlated, so MI is far from 0
        crop = mask is not None
        crit = RefNMI(list(centers), device='cpu', sigma_ratio=ratio, max_clip=maxc, crop_background=crop)
        loss = crit(yt, yp, mask=mask) if crop else crit(yt, yp)
        loss.backward()
        out.update({tag + "_true": npy(yt), tag + "_pred": npy(yp), tag + "_centers": np.asarray(centers, np.float64),
                    tag + "_params": np.array([ratio, maxc, float(crop)]), tag + "_loss": npy(loss),
                    tag + "_dtrue": npy(yt.grad), tag + "_dpred": npy(yp.grad)})
        if crop:
            out[tag + "_mask"] = npy(mask)
        print("%-16s loss %s" % (tag, npy(loss)))
    out["cases"] = np.array([c[0] for c in cases()])
    MG.HERE = HERE
    MG.save("nmi.npz", **out)


if __name__ == "__main__":
    main()
