"""Generator of tests/golden/hausdorff.npz -- the reference's HausdorffDistance (util/loss_metrics.py:105-132: scipy's
distance_transform_edt on the host) on seeded blocky binary masks.  Runs only where the reference checkout
(make_golden.REF) and scipy exist; imports the reference itself with the shims of make_golden.py plus two more: a stub
`torchvision.models` (the file imports it for a VGG it does not use here) and `np.Inf`, which NumPy 2 removed.  Records the
inputs as 8-bit masks [B,1,*vol] and the reference's own output, per case <nd>d_<case> for nd = 2 ((37, 70)) and 3
((21, 33, 70)), B = 1:

  overlap      two overlapping blocky blobs          disjoint     blobs in opposite halves
  identical    the same mask twice (0)               corners      one voxel each in opposite corners (d2 = sum (n - 1)^2)
  empty_pred   no voxel in pred (inf)                ring_disc    a ring in target around a disc in pred: the maximum
                                                                  lies at an interior voxel of the disc
  <tag>_pred, <tag>_target (uint8), <tag>_hd (float32)

and the batch-mixing case mix_pred, mix_target [2,1,12,16] with mix_ref_hd: sample 0 holds only pred, sample 1 only target.
The reference runs the transform over the whole [B,1,*vol] array, so the batch axis counts as a spatial axis and it
answers a finite distance; the tree scores every sample on its own ([inf, inf]) -- the documented divergence.

    python tests/golden/make_golden_hausdorff.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests.golden import make_golden as MG                                # noqa: E402
from tests.test_hausdorff import FIXTURE_CASES, _ring_disc, blocky_labels  # noqa: E402

VOLS = {2: (37, 70), 3: (21, 33, 70)}


def masks(nd, case, seed):
    vol = VOLS[nd]
    shape = (1, 1) + vol
    if case == "ring_disc":
        return _ring_disc(vol)
    a = blocky_labels(seed, 1, vol, 3, 5).numpy() == 1
    b = blocky_labels(seed + 1, 1, vol, 3, 5).numpy() == 1
    half = vol[-1] // 2
    if case == "overlap":
        return a, a & b | np.roll(a, 4, axis=-1)
    if case == "disjoint":
        a[..., half - 3:] = False
        b[..., :half + 3] = False
        return a, b
    if case == "identical":
        return a, a.copy()
    if case == "corners":
        p, t = np.zeros(shape, bool), np.zeros(shape, bool)
        p[(0, 0) + (0,) * nd] = True
        t[(0, 0) + tuple(n - 1 for n in vol)] = True
        return p, t
    if case == "empty_pred":
        return np.zeros(shape, bool), b
    raise KeyError(case)


def main():
    MG.install_shims()
    tv = sys.modules["torchvision"]
    tv.models = sys.modules.setdefault("torchvision.models", types.ModuleType("torchvision.models"))
    if not hasattr(np, "Inf"):
        np.Inf = np.inf
    if MG.REF not in sys.path:
        sys.path.insert(0, MG.REF)
    from util.loss_metrics import HausdorffDistance as RefHD
    ref = RefHD()
    out = {}
    for nd in (2, 3):
        for i, case in enumerate(FIXTURE_CASES):
            tag = "%dd_%s" % (nd, case)
            p, t = masks(nd, case, 700 + 100 * nd + 10 * i)
            hd = ref.compute(torch.from_numpy(p.astype(np.float32)), torch.from_numpy(t.astype(np.float32)))
            out[tag + "_pred"], out[tag + "_target"] = p.astype(np.uint8), t.astype(np.uint8)
            out[tag + "_hd"] = np.float32(float(hd.reshape(-1)[0]))
            print("%-14s |pred| %6d |target| %6d  hd %s" % (tag, p.sum(), t.sum(), out[tag + "_hd"]))
    p, t = np.zeros((2, 1, 12, 16), bool), np.zeros((2, 1, 12, 16), bool)
    p[0, 0, 2:4, 3:5] = True
    t[1, 0, 9:11, 10:12] = True
    hd = ref.compute(torch.from_numpy(p.astype(np.float32)), torch.from_numpy(t.astype(np.float32)))
    out["mix_pred"], out["mix_target"] = p.astype(np.uint8), t.astype(np.uint8)
    out["mix_ref_hd"] = np.float32(float(hd.reshape(-1)[0]))
    print("mix            reference (across the batch axis) %s" % out["mix_ref_hd"])
    out["cases"] = np.array(FIXTURE_CASES)
    MG.HERE = HERE
    MG.save("hausdorff.npz", **out)


if __name__ == "__main__":
    main()
