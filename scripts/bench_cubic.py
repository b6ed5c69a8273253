"""GPU box: cubic B-spline resampling (dfmir_amd/csrc/cubic.hip) at 160x192x224 (1 channel) and at 2-D 256x256, batch 16, in one
process:

  (a) ops.spline_prefilter beside ops.gaussian_smooth at sigma 16 / 3 (the same radius, 16), the two alternating, with the
      achieved fraction of 8 TB/s on the bytes of the crossings: 3-D two reads and two writes of the tensor (the (y, x) pass and
      the z pass), 2-D one read and one write;
  (b) ops.warp_cubic(prefiltered=True) forward, and forward + backward to the flow, beside ops.warp linear forward and forward +
      backward to the flow, on the same image and flow (flows of up to 1.5 voxels), with the fraction of 8 TB/s on the bytes a
      forward needs (image and flow read once, the result written once);
  (c) ops.warp_cubic with prefiltered=False (the prefilter in every call) beside prefiltered=True.

HIP-event timed per call, medians over `--reps` calls after a warm-up, over a rotating set of inputs whose total exceeds the
256 MiB last-level cache (cold buffers); the candidates alternate inside the one process, three rounds each.

    python scripts/bench_cubic.py [--reps 20] [--out profiles/cubic_timing.txt]
"""
import argparse
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from scripts.bench_demons import alternate  # noqa: E402

DEV = "cuda"
HBM = 8.0e12
CASES = (("3-D", (1, 1, 160, 192, 224), 12), ("2-D", (16, 1, 256, 256), 72))       # (tag, image shape, buffers in rotation)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cubic_timing.txt"))
    args = ap.parse_args()
    import torch
    from dfmir_amd import ops
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device=DEV).manual_seed(1)
    emit("cubic B-spline resampling on %s (scripts/bench_cubic.py --reps %d)" % (torch.cuda.get_device_name(0), args.reps))
    emit("medians of 3 alternating rounds x %d calls, HIP events; every input comes from a rotating set larger than the 256 MiB cache" % args.reps)
    for tag, shape, n in CASES:
        nd = len(shape) - 2
        numel = math.prod(shape)
        name = "x".join(map(str, shape))
        imgs = [torch.rand(*shape, device=DEV, generator=g) * 2 - 1 for _ in range(n)]
        flows = [(torch.rand(shape[0], nd, *shape[2:], device=DEV, generator=g) * 2 - 1) * 1.5 for _ in range(n)]
        gflows = [f.clone().requires_grad_() for f in flows]
        emit()
        cross = 2 if nd == 3 else 1
        emit("%s (a) ops.spline_prefilter, image %s (%.1f MB; %d read + %d write of the tensor)" % (tag, name, 4e-6 * numel, cross, cross))
        res = alternate({"ops.spline_prefilter": lambda i: ops.spline_prefilter(imgs[i % n]),
                         "ops.gaussian_smooth sigma 16/3": lambda i: ops.gaussian_smooth(imgs[i % n], 16.0 / 3.0)}, args.reps)
        for k, (t, rounds) in res.items():
            emit("    %-36s %8.4f ms   %.3f of 8 TB/s   rounds %s" % (k, t, 2 * cross * 4.0 * numel / (t * 1e-3) / HBM, ["%.4f" % v for v in rounds]))
        emit("    prefilter / Gaussian = %.2f x" % (res["ops.spline_prefilter"][0] / res["ops.gaussian_smooth sigma 16/3"][0]))

        coefs = [ops.spline_prefilter(x) for x in imgs]
        nbytes = 4.0 * numel * (2 + nd)
        emit("%s (b) warps of %s, flows of up to 1.5 voxels (bytes of a forward: image, flow in, result out = %.0f MB)" % (tag, name, nbytes * 1e-6))
        ones = torch.ones(*shape, device=DEV)
        res = alternate({
            "warp_cubic forward (prefiltered)": lambda i: ops.warp_cubic(coefs[i % n], flows[i % n], prefiltered=True),
            "warp linear forward": lambda i: ops.warp(imgs[i % n], flows[i % n]),
            "warp_cubic forward + backward": lambda i: torch.autograd.grad(ops.warp_cubic(coefs[i % n], gflows[i % n], prefiltered=True), gflows[i % n], ones),
            "warp linear forward + backward": lambda i: torch.autograd.grad(ops.warp(imgs[i % n], gflows[i % n]), gflows[i % n], ones)}, args.reps)
        for k, (t, rounds) in res.items():
            emit("    %-36s %8.4f ms   %.3f of 8 TB/s   rounds %s" % (k, t, nbytes / (t * 1e-3) / HBM, ["%.4f" % v for v in rounds]))
        emit("    cubic / linear: forward %.2f x,  forward + backward %.2f x"
             % (res["warp_cubic forward (prefiltered)"][0] / res["warp linear forward"][0],
                res["warp_cubic forward + backward"][0] / res["warp linear forward + backward"][0]))

        emit("%s (c) ops.warp_cubic, the prefilter in the call against prefiltered=True" % tag)
        res = alternate({"warp_cubic (prefilters)": lambda i: ops.warp_cubic(imgs[i % n], flows[i % n]),
                         "warp_cubic prefiltered=True": lambda i: ops.warp_cubic(coefs[i % n], flows[i % n], prefiltered=True)}, args.reps)
        for k, (t, rounds) in res.items():
            emit("    %-36s %8.4f ms   rounds %s" % (k, t, ["%.4f" % v for v in rounds]))
        emit("    default / prefiltered = %.2f x" % (res["warp_cubic (prefilters)"][0] / res["warp_cubic prefiltered=True"][0]))
        del imgs, flows, gflows, coefs, ones
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
