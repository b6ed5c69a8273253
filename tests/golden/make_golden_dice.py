"""Generator of tests/golden/dice.npz -- the reference's vxm `Dice` / `MSE` (models/voxelmorph/torchvoxelmorph/losses.py:70-90)
and its `SpatialTransformer` (layers.py:6-48) on seeded inputs.  Runs only where the reference checkout (make_golden.REF)
exists; imports the reference itself with the shims of make_golden.py and records inputs + the reference's own outputs.

Label cases <tag> (the one-hot composition `Dice().loss(one_hot(fix)[:, labels], SpatialTransformer(one_hot(mov)[:, labels],
flow))`, autograd through both):
  <tag>_mov, <tag>_fix      uint8 label maps [B,1,*vol]
  <tag>_flow, <tag>_labels  fp32 flow [B,nd,*vol] (pushes corners out of the volume on every face); the scored values
  <tag>_mode                0 bilinear, 1 nearest (forward only)
  <tag>_loss, <tag>_dice    the loss and 2 top / bottom per (b, l)
  <tag>_dflow               d loss / d flow (bilinear cases)
No sampling coordinate x + flow lies within 1e-3 of an integer along any axis (asserted; offending flow values are nudged):
d(flow) of a multi-linear sample jumps at cell boundaries, and the reference reaches its coordinate through a
normalise / de-normalise round trip.  The nearest case keeps the same distance from the half-integers.

Dense cases <tag>: <tag>_true, <tag>_pred -> <tag>_dice_loss / _dice_dtrue / _dice_dpred and <tag>_mse_loss / _mse_dtrue /
_mse_dpred.

    python tests/golden/make_golden_dice.py
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

EPS = 1e-3


def label_map(seed, B, vol, nvals, block):
    """Blocky random labels in [0, nvals): a coarse random grid repeated `block` times per axis, then ~20 % of the voxels
    redrawn one by one (so corners of one voxel carry the same label often, and different ones often)."""
    coarse = [(-(-s // block)) for s in vol]
    x = (C.rand(seed, B, 1, *coarse) * nvals).long().clamp_(max=nvals - 1)
    for ax in range(len(vol)):
        x = x.repeat_interleave(block, dim=2 + ax)
    x = x[(slice(None), slice(None)) + tuple(slice(0, s) for s in vol)]
    noise = (C.rand(seed + 1, B, 1, *vol) * nvals).long().clamp_(max=nvals - 1)
    return torch.where(C.rand(seed + 2, B, 1, *vol) < 0.2, noise, x).to(torch.uint8).contiguous()


def make_flow(seed, B, vol, amp, nearest):
    """Uniform displacements in [-amp, amp]; coordinates nudged away from the integers (and, for the nearest case, from the
    half-integers) by more than EPS, evaluated in fp32 as the kernel does."""
    nd = len(vol)
    flow = ((C.rand(seed, B, nd, *vol) * 2 - 1) * amp).float()
    grid = torch.stack(torch.meshgrid([torch.arange(s, dtype=torch.float32) for s in vol], indexing='ij'))[None]
    for _ in range(8):
        p = grid + flow
        frac = p - torch.floor(p)
        bad = (frac < 2 * EPS) | (frac > 1 - 2 * EPS)
        if nearest:
            bad |= (frac - 0.5).abs() < 2 * EPS
        if not bool(bad.any()):
            break
        flow = torch.where(bad, flow + 0.0137, flow)
    p = (grid + flow).double()
    frac = p - torch.floor(p)
    assert float(torch.minimum(frac, 1 - frac).min()) > EPS, "a sampling coordinate lies within 1e-3 of an integer"
    if nearest:
        assert float((frac - 0.5).abs().min()) > EPS
    for ax, s in enumerate(vol):                       # corners leave the volume on every face
        assert float(p[:, ax].min()) < -1.0 and float(p[:, ax].max()) > s, (ax, float(p[:, ax].min()), float(p[:, ax].max()))
    return flow.contiguous()


def one_hot(x, labels):
    return torch.cat([(x == int(l)).float() for l in labels], 1)


def label_cases():
    """(tag, B, vol, values in the maps, block, labels, flow amplitude, nearest, label removed from mov or None)"""
    return [
        ("2d_b2_k3_skip_background", 2, (24, 21), 5, 3, [1, 2, 3], 3.5, False, None),
        ("2d_b1_k1_w4", 1, (16, 24), 3, 4, [2], 3.0, False, None),
        ("3d_b1_k6_absent", 1, (10, 12, 14), 6, 2, [1, 2, 3, 4, 7, 200], 3.0, False, 4),
        ("3d_b2_k64_w4", 2, (9, 11, 16), 80, 2, list(range(1, 65)), 3.0, False, None),
        ("3d_b1_k35_w4", 1, (8, 12, 16), 36, 3, list(range(1, 36)), 2.5, False, None),
        ("3d_b2_nearest", 2, (10, 12, 14), 7, 2, [0, 1, 2, 3, 5, 9], 3.0, True, None),
    ]


def dense_cases():
    return [("dense_2d", (2, 4, 18, 22)), ("dense_3d", (1, 5, 8, 10, 12)), ("dense_3d_w4", (2, 3, 6, 8, 16))]


def main():
    MG.install_shims()
    from models.voxelmorph.torchvoxelmorph.layers import SpatialTransformer as RefST
    from models.voxelmorph.torchvoxelmorph.losses import Dice as RefDice
    from models.voxelmorph.torchvoxelmorph.losses import MSE as RefMSE
    npy = MG.npy
    out = {}
    for i, (tag, B, vol, nvals, block, labels, amp, nearest, drop) in enumerate(label_cases()):
        mov = label_map(300 + 10 * i, B, vol, nvals, block)
        fix = label_map(305 + 10 * i, B, vol, nvals, block)
        fix = torch.where(C.rand(309 + 10 * i, *fix.shape) < 0.5, mov, fix)       # overlapping, so Dice is far from 0
        if drop is not None:
            mov = torch.where(mov == drop, torch.zeros_like(mov), mov)
            assert bool((fix == drop).any()) and not bool((mov == drop).any())
        flow = make_flow(307 + 10 * i, B, vol, amp, nearest).requires_grad_(not nearest)
        t = one_hot(fix, labels)
        p = RefST(vol, mode='nearest' if nearest else 'bilinear')(one_hot(mov, labels), flow)
        loss = RefDice().loss(t, p)
        axes = list(range(2, 2 + len(vol)))
        dice = 2 * (t * p).sum(dim=axes) / torch.clamp((t + p).sum(dim=axes), min=1e-5)
        out.update({tag + "_mov": npy(mov), tag + "_fix": npy(fix), tag + "_flow": npy(flow),
                    tag + "_labels": np.asarray(labels, np.int64), tag + "_mode": np.array(int(nearest)),
                    tag + "_loss": npy(loss), tag + "_dice": npy(dice)})
        if not nearest:
            loss.backward()
            out[tag + "_dflow"] = npy(flow.grad)
        print("%-26s loss %.6f  dice min %.4f max %.4f" % (tag, float(loss.detach()), float(dice.min()), float(dice.max())))
    for i, (tag, shape) in enumerate(dense_cases()):
        t0 = (C.rand(400 + 10 * i, *shape) > 0.6).float()
        p0 = (0.5 * t0 + 0.5 * C.rand(401 + 10 * i, *shape))
        t0[:, 1] = 0.0                                                # a channel empty in both: the clamp is active
        p0[:, 1] = 0.0
        out.update({tag + "_true": npy(t0), tag + "_pred": npy(p0)})
        for name, crit in (("dice", RefDice()), ("mse", RefMSE())):
            t, p = t0.clone().requires_grad_(), p0.clone().requires_grad_()
            loss = crit.loss(t, p)
            loss.backward()
            out.update({"%s_%s_loss" % (tag, name): npy(loss), "%s_%s_dtrue" % (tag, name): npy(t.grad),
                        "%s_%s_dpred" % (tag, name): npy(p.grad)})
            print("%-26s %s %.6f" % (tag, name, float(loss)))
    out["cases"] = np.array([c[0] for c in label_cases()])
    out["dense_cases"] = np.array([c[0] for c in dense_cases()])
    MG.HERE = HERE
    MG.save("dice.npz", **out)


if __name__ == "__main__":
    main()
