"""GPU box: NMI_Loss (util/losses.py:263-348) forward and backward, HIP kernels (dfmir_amd.ops.nmi_loss) against the same
formula as eager torch ops on the same card, at 128^3 and 160x192x224 for nb in {32, 64}.  HIP-event timed over a
rotating set of inputs.  GFLOP/s counts the matrix work only -- forward 2 nb^2 V (the joint histogram), backward 4 nb^2 V
(the two nb x nb matrix-vector products per voxel) -- and is set against the 157.3 TF fp32 matrix peak.

    python scripts/bench_nmi.py [--reps 20] [--out profiles/nmi_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dfmir_amd import ops

PEAK_TF = 157.3
DEV = "cuda"


def eager_nmi(y_true, y_pred, centers, preterm, max_clip=1.0):
    """The reference's formula (util/losses.py:319-348) as eager torch ops -- the comparison row, not the product path."""
    yt = torch.clamp(y_true, 0, max_clip).view(1, 1, -1)
    yp = torch.clamp(y_pred, 0, max_clip).view(1, 1, -1)
    vbc = centers.view(1, -1, 1)
    ia = torch.exp(-preterm * (yt - vbc) ** 2)
    ia = ia / torch.sum(ia, dim=1, keepdim=True)
    ib = torch.exp(-preterm * (yp - vbc) ** 2)
    ib = ib / torch.sum(ib, dim=1, keepdim=True)
    pab = torch.bmm(ib, ia.transpose(1, 2)) / yt.shape[2]
    pa = torch.mean(ia, dim=-1, keepdim=True)
    pb = torch.mean(ib, dim=-1, keepdim=True)
    papb = torch.bmm(pb, pa.transpose(1, 2)) + 1e-5
    return -torch.sum(pab * torch.log(pab / papb + 1e-5), dim=(1, 2))


def timeit(fn, reps):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(reps):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for shape in ((128, 128, 128), (160, 192, 224)):
        V = int(np.prod(shape))
        xs = [torch.rand(1, 1, *shape, device=DEV).requires_grad_() for _ in range(3)]
        ys = [(0.5 * x.detach() + 0.5 * torch.rand_like(x)).requires_grad_() for x in xs]
        for nb in (32, 64):
            centers = np.linspace(0.0, 1.0, nb)
            preterm = ops.nmi_preterm(centers)
            cdev = torch.tensor(centers, dtype=torch.float32, device=DEV)
            row = {"shape": list(shape), "nb": nb, "voxels": V}
            for impl, f in (("hip", lambda a, b: ops.nmi_loss(a, b, centers)),
                            ("eager_torch", lambda a, b: eager_nmi(a, b, cdev, preterm))):
                with torch.no_grad():
                    fwd = timeit(lambda i: f(xs[i % 3], ys[i % 3]), args.reps)
                losses = [f(x, y) for x, y in zip(xs, ys)]
                bwd = timeit(lambda i: torch.autograd.grad(losses[i % 3], (xs[i % 3], ys[i % 3]), retain_graph=True),
                             args.reps)
                del losses
                torch.cuda.empty_cache()
                gf, gb = 2.0 * nb * nb * V / fwd / 1e6, 4.0 * nb * nb * V / bwd / 1e6
                row[impl] = {"fwd_ms": round(fwd, 4), "bwd_ms": round(bwd, 4), "fwd_gflops": round(gf, 1),
                             "bwd_gflops": round(gb, 1), "fwd_peak_frac": round(gf / (PEAK_TF * 1e3), 4),
                             "bwd_peak_frac": round(gb / (PEAK_TF * 1e3), 4)}
                print("%-12s %-14s nb %2d  fwd %8.3f ms (%7.1f GFLOP/s, %5.1f %% of peak)  bwd %8.3f ms (%7.1f GFLOP/s, "
                      "%5.1f %%)" % (impl, "x".join(map(str, shape)), nb, fwd, gf, 100 * gf / (PEAK_TF * 1e3), bwd, gb,
                                      100 * gb / (PEAK_TF * 1e3)), flush=True)
            rows.append(row)
        del xs, ys
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "peak_tflops_f32": PEAK_TF, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
