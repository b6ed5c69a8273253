"""GPU box: the label-map Dice under a flow (dfmir_amd.ops.warp_dice, csrc/dice.hip) at 160x192x224 with K = 35 labels:
the fused forward and backward; the composition the tree could run before it -- torch one-hot of both label maps, ops.warp
of the K-channel volume, the Dice formula in eager torch, forward + backward -- in the same process; and the
Registration3DModel step with and without the segmentation term.  HIP-event timed per call, medians over `--reps` calls
after a warm-up, over a rotating set of flows larger than the 256 MB last-level cache so that the flow is read cold.
The fused forward's bytes (flow + both label maps, read once) are set against the 8 TB/s HBM figure of bench.py's warp
roofline.

    python scripts/bench_dice.py [--reps 20] [--out profiles/dice_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dfmir_amd import ops
from dfmir_amd.registration3d import Registration3DModel

HBM_TBS = 8.0
DEV = "cuda"
NBUF = 4                     # 4 x 82.6 MB of flow > the 256 MB last-level cache


def labels_like(shape, nvals, block, seed):
    g = torch.Generator().manual_seed(seed)
    coarse = [-(-s // block) for s in shape]
    x = (torch.rand(1, 1, *coarse, generator=g) * nvals).long().clamp_(max=nvals - 1)
    for ax in range(3):
        x = x.repeat_interleave(block, dim=2 + ax)
    return x[:, :, :shape[0], :shape[1], :shape[2]].to(torch.uint8).contiguous()


def one_hot(x, labels):
    return torch.cat([(x == int(l)).float() for l in labels], 1)


def eager_composition(mov, fix, flow, labels):
    """What the tree could compose before the fused kernels: one-hot, ops.warp of K channels, the Dice formula in torch."""
    t = one_hot(fix, labels)
    p = ops.warp(one_hot(mov, labels), flow)
    top = 2 * (t * p).sum(dim=(2, 3, 4))
    bottom = torch.clamp((t + p).sum(dim=(2, 3, 4)), min=1e-5)
    return -torch.mean(top / bottom)


def median_ms(fn, reps, warm=3):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    ts = []
    for i in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn(warm + i)
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    shape, K = (160, 192, 224), 35
    V = int(np.prod(shape))
    labels = list(range(1, K + 1))
    mov = labels_like(shape, K + 5, 8, 1).to(DEV)
    fix = torch.where(torch.rand(1, 1, *shape, device=DEV) < 0.7, mov, labels_like(shape, K + 5, 8, 2).to(DEV))
    flows = [((torch.rand(1, 3, *shape, device=DEV) * 2 - 1) * 3.0).requires_grad_() for _ in range(NBUF)]
    res = {"shape": list(shape), "K": K, "voxels": V}

    with torch.no_grad():
        fwd = median_ms(lambda i: ops.warp_dice(mov, fix, flows[i % NBUF], labels), args.reps)
    losses = [ops.warp_dice(mov, fix, f, labels)[0] for f in flows]
    bwd = median_ms(lambda i: torch.autograd.grad(losses[i % NBUF], flows[i % NBUF], retain_graph=True), args.reps)
    both = median_ms(lambda i: torch.autograd.grad(ops.warp_dice(mov, fix, flows[i % NBUF], labels)[0], flows[i % NBUF]),
                     args.reps)
    del losses
    fwd_bytes = V * (3 * 4 + 2)
    bwd_bytes = V * (3 * 4 * 2 + 2)
    res["fused"] = {"fwd_ms": round(fwd, 4), "bwd_ms": round(bwd, 4), "fwd_bwd_ms": round(both, 4),
                    "fwd_bytes": fwd_bytes, "fwd_tbs": round(fwd_bytes / fwd / 1e9, 3),
                    "fwd_hbm_frac": round(fwd_bytes / fwd / 1e9 / HBM_TBS, 4),
                    "bwd_bytes": bwd_bytes, "bwd_tbs": round(bwd_bytes / bwd / 1e9, 3),
                    "bwd_hbm_frac": round(bwd_bytes / bwd / 1e9 / HBM_TBS, 4)}
    print("fused        fwd %8.3f ms (%.2f TB/s, %4.1f %% of %g TB/s)  bwd %8.3f ms (%.2f TB/s, %4.1f %%)  fwd+bwd %8.3f ms"
          % (fwd, fwd_bytes / fwd / 1e9, 100 * fwd_bytes / fwd / 1e9 / HBM_TBS, HBM_TBS, bwd, bwd_bytes / bwd / 1e9,
             100 * bwd_bytes / bwd / 1e9 / HBM_TBS, both), flush=True)

    reps_e = max(3, args.reps // 4)
    with torch.no_grad():
        efwd = median_ms(lambda i: eager_composition(mov, fix, flows[i % NBUF], labels), reps_e, warm=2)
    eboth = median_ms(lambda i: torch.autograd.grad(eager_composition(mov, fix, flows[i % NBUF], labels), flows[i % NBUF]),
                      reps_e, warm=2)
    torch.cuda.empty_cache()
    res["one_hot_composition"] = {"fwd_ms": round(efwd, 3), "fwd_bwd_ms": round(eboth, 3)}
    res["speedup"] = {"fwd": round(efwd / fwd, 1), "fwd_bwd": round(eboth / both, 1)}
    print("composition  fwd %8.3f ms  fwd+bwd %8.3f ms   -> fused is %.1fx / %.1fx faster"
          % (efwd, eboth, efwd / fwd, eboth / both), flush=True)
    del flows
    torch.cuda.empty_cache()

    if not args.no_model:
        A = torch.rand(1, 1, *shape, device=DEV)
        B = 0.5 * A + 0.5 * torch.rand(1, 1, *shape, device=DEV)
        for name, kw in (("step_ncc", {}), ("step_ncc_dice", {"seg_labels": labels, "seg_weight": 1.0})):
            torch.manual_seed(0)
            m = Registration3DModel(shape, device=DEV, **kw)
            data = {"A": A, "B": B, "A_seg": mov, "B_seg": fix}

            def step(i):
                m.set_input(data)
                m.optimize_parameters()
            ms = median_ms(step, max(5, args.reps // 2), warm=3)
            res[name + "_ms"] = round(ms, 3)
            print("%-14s %8.3f ms per step" % (name, ms), flush=True)
            del m
            torch.cuda.empty_cache()
        res["step_dice_cost_ms"] = round(res["step_ncc_dice_ms"] - res["step_ncc_ms"], 3)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "hbm_tbs": HBM_TBS, "result": res}, fh, indent=1)


if __name__ == "__main__":
    main()
