"""GPU box: the warped-feature SSD (dfmir_amd.ops.warp_ssd, csrc/warpssd.hip) at 1x12x160x192x224 and 16x4x256x256, per call:
forward + flow gradient of the fused op on the packed gather and, with DFMIR_WARPSSD_PLANAR set, on the channel-major one,
beside the composition it replaces -- ops.warp -> ops.mse_loss -> backward to the flow -- on the same inputs, the three
alternating in one process; the fused forward alone; the pack; and a whole infer.refine_flow iteration (MIND-sized user
features, the diffusion penalty, grid_downsize 2) as (time of 10 iterations - time of 0 iterations) / 10.

HIP-event timed per call, medians over `--reps` calls after a warm-up, over a rotating set of inputs (every feature tensor of
the 3-D shape is larger than the 256 MiB last-level cache).  The flow is registration-like: a smooth displacement of up to 3
voxels (noise at 1/8 resolution, linearly up-sampled); the features are noise in [0, 1].  Algorithmic traffic per voxel of the
fused pass: C floats of F and nd of phi read, nd of the gradient written, and the gathered corners of M, which neighbouring
voxels share (about Cp floats per voxel from HBM, the rest from L2): 4 * (2 C + 2 nd) bytes, against three times the feature
bytes for the composition (the warped tensor written, read, its gradient written and read).

    python scripts/bench_refine.py [--reps 20] [--out profiles/refine_timing.txt]
"""
import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_TBS = 8.0
DEV = "cuda"
SHAPES = {"1x12x160x192x224": (1, 12, 160, 192, 224), "16x4x256x256": (16, 4, 256, 256)}
SETS = 2


def median_ms(fn, reps, warm=3):
    import torch
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


def make_inputs(shape):
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device=DEV).manual_seed(1)
    B, vol = shape[0], shape[2:]
    nd = len(vol)
    out = []
    for _ in range(SETS):
        low = [max(2, s // 8) for s in vol]
        phi = F.interpolate(torch.rand(B, nd, *low, device=DEV, generator=g) * 6.0 - 3.0, size=vol,
                            mode='trilinear' if nd == 3 else 'bilinear', align_corners=True).contiguous()
        M = torch.rand(*shape, device=DEV, generator=g)
        Fx = torch.rand(*shape, device=DEV, generator=g)
        out.append((M, Fx, phi.requires_grad_()))
    return out


def bench_shape(name, reps, emit):
    import torch
    from dfmir_amd import _lib, infer, ops
    shape = SHAPES[name]
    B, Cn, vol = shape[0], shape[1], shape[2:]
    nd, S = len(vol), math.prod(shape[2:])
    sets = make_inputs(shape)
    handles = [ops.pack_features(M) for M, _, _ in sets]
    n = len(sets)

    def fused(i):
        _, Fx, phi = sets[i % n]
        return torch.autograd.grad(ops.warp_ssd(handles[i % n], Fx, phi), phi)

    def fused_fwd(i):
        _, Fx, phi = sets[i % n]
        with torch.no_grad():
            return ops.warp_ssd(handles[i % n], Fx, phi)

    def composed(i):
        M, Fx, phi = sets[i % n]
        return torch.autograd.grad(ops.mse_loss(Fx, ops.warp(M, phi)), phi)

    acc = {k: [] for k in ("fused packed", "fused planar", "warp + mse + backward")}
    for _ in range(3):                                   # the three alternate, three rounds each
        for tag in acc:
            _lib.set_option("DFMIR_WARPSSD_PLANAR", "1" if tag == "fused planar" else None)
            acc[tag].append(median_ms(composed if tag.startswith("warp") else fused, reps))
    _lib.set_option("DFMIR_WARPSSD_PLANAR", None)
    fwd = median_ms(fused_fwd, reps)
    pack = median_ms(lambda i: ops.pack_features(sets[i % n][0]), reps)
    # the fused value and gradient are the composition's
    a, b = fused(0)[0], composed(0)[0]
    agree = float((a - b).abs().max() / b.abs().max())
    traffic = 4.0 * B * S * (2 * Cn + 2 * nd)
    emit("%s  (B x C x vol; %d input sets, medians of 3 rounds x %d calls)" % (name, n, reps))
    for tag, v in acc.items():
        med = statistics.median(v)
        extra = ""
        if tag.startswith("fused"):
            extra = "   %.0f MB algorithmic -> %.2f TB/s, %.0f %% of the %.0f TB/s HBM peak" % (
                traffic / 1e6, traffic / med / 1e9, 100.0 * traffic / med / 1e9 / HBM_TBS, HBM_TBS)
        emit("  %-24s forward + dflow  %8.4f ms   rounds %s%s" % (tag, med, ["%.4f" % x for x in v], extra))
    ratio = statistics.median(acc["warp + mse + backward"]) / statistics.median(acc["fused packed"])
    emit("  composition / fused packed = %.2f x;  planar / packed = %.2f x;  dflow fused vs composition, max-abs over max: %.2e"
         % (ratio, statistics.median(acc["fused planar"]) / statistics.median(acc["fused packed"]), agree))
    emit("  %-24s forward only     %8.4f ms" % ("fused packed", fwd))
    emit("  %-24s once per loop    %8.4f ms" % ("pack_features", pack))
    M, Fx, phi = sets[0]
    img = M[:, :1].contiguous()
    kw = dict(features=(M, Fx), lam=0.05, lr=0.1, grid_downsize=2)
    loop = lambda it: median_ms(lambda i: infer.refine_flow(img, img, phi.detach(), iters=it, **kw), max(3, reps // 4), warm=1)
    t0, t10 = loop(0), loop(10)
    emit("  %-24s per iteration    %8.4f ms   (10 iterations %.3f ms, set-up + final evaluation %.3f ms)"
         % ("infer.refine_flow", (t10 - t0) / 10.0, t10, t0))
    emit("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "refine_timing.txt"))
    args = ap.parse_args()
    import torch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("warped-feature SSD and instance optimisation on %s (scripts/bench_refine.py --reps %d)"
         % (torch.cuda.get_device_name(0), args.reps))
    emit("")
    for name in SHAPES:
        bench_shape(name, args.reps, emit)
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
