"""profiles/tps_timing.txt: ops.tps_flow forward and backward (dfmir_amd/csrc/tps.hip) at the workload volume 160 x 192 x 224
with K = 256 / 1024 / 4096 control points and at 256^2 in 2-D, beside the eager composition it replaces (chunked pairwise
distances + matmul in fp32, which never holds more than `--chunk` rows of the N x K matrix) and ops.bspline_flow at the same
volume.  Needs the GPU; times are device events around `--reps` calls after `--warmup` calls, the median of `--rounds` rounds.

    python scripts/bench_tps.py [--out profiles/tps_timing.txt] [--label TEXT]

Share of peak: the pair sum needs, per (voxel, control point) pair, nd float64 FMAs (2 nd FLOP) and about 3 nd + 1 fp32
operations for the squared distance and phi (2-D: + log); the fp64 figure is 2 nd pairs / time over the 78.6 TFLOP/s fp64
vector peak of the MI355X, the fp32 figure (3 nd + 1) pairs / time over its 157.3 TFLOP/s.  The kernel is bound by the sum
of the two streams through one vector pipe, so neither share alone can reach 1.  Another build of the same C ABI (an A/B
experiment on the kernel) is timed through DFMIR_HIP_LIB=<that library>, `--label` and `--no-eager`."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from dfmir_amd import ops  # noqa: E402

PEAK64, PEAK32 = 78.6e12, 157.3e12


def timed(fn, warmup, reps, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return statistics.median(ms), min(ms), max(ms)


def phi32(s, nd):
    if nd == 3:
        return -s.sqrt()
    return torch.where(s > 0, 0.5 * s * torch.log(s.clamp_min(1e-38)), torch.zeros_like(s))


def eager_basis(xh, qh, nd):
    s = torch.zeros(xh.shape[0], qh.shape[0], device=xh.device)
    for a in range(nd):
        s += (xh[:, a, None] - qh[None, :, a]).square()
    return phi32(s, nd)


def eager_forward(coef32, qh, grid_fn, N, K, nd, chunk):
    out = torch.empty(N, nd, device=qh.device)
    for i in range(0, N, chunk):
        xh = grid_fn(i, min(N, i + chunk))
        out[i:i + chunk] = eager_basis(xh, qh, nd) @ coef32[:K] + coef32[K] + xh @ coef32[K + 1:]
    return out


def eager_backward(g, qh, grid_fn, N, K, nd, chunk):
    dc = torch.zeros(K + nd + 1, nd, device=qh.device)
    for i in range(0, N, chunk):
        xh = grid_fn(i, min(N, i + chunk))
        gi = g[i:i + chunk]
        dc[:K] += eager_basis(xh, qh, nd).t() @ gi
        dc[K] += gi.sum(0)
        dc[K + 1:] += xh.t() @ gi
    return dc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tps_timing.txt"))
    ap.add_argument("--label", default="the in-tree build")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 16)
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tps.py measures on the GPU"
    dev = "cuda"
    lines = ["# ops.tps_flow on %s -- %s" % (torch.cuda.get_device_name(0), args.label),
             "# ms per call: median (min .. max) of %d rounds of %d calls after %d warm-up calls" % (args.rounds, args.reps, args.warmup),
             "%-16s %5s %-22s %9s %19s %9s %7s %7s" % ("volume", "K", "what", "ms", "(min .. max)", "Gpair/s", "fp64", "fp32")]

    def row(vol, K, what, t, pairs=None, nd=3):
        med, lo, hi = t
        if pairs:
            rate = pairs / (med * 1e-3)
            extra = "%9.1f %6.1f%% %6.1f%%" % (rate / 1e9, 100 * 2 * nd * rate / PEAK64, 100 * (3 * nd + 1) * rate / PEAK32)
        else:
            extra = "%9s %7s %7s" % ("-", "-", "-")
        lines.append("%-16s %5s %-22s %9.3f %19s %s" % ("x".join(map(str, vol)), K, what, med, "(%.3f .. %.3f)" % (lo, hi), extra))
        print(lines[-1], flush=True)

    for vol, Ks in (((160, 192, 224), (256, 1024, 4096)), ((256, 256), (1024,))):
        nd = len(vol)
        N = 1
        for n in vol:
            N *= n
        gen = torch.Generator().manual_seed(0)
        g = torch.randn(1, nd, *vol, generator=gen).to(dev)
        for K in Ks:
            ext = torch.tensor([n - 1.0 for n in vol])
            q = (torch.rand(1, K, nd, generator=gen) * ext).to(dev)
            p = q + torch.randn(1, K, nd, generator=gen).to(dev)
            fit = ops.tps_fit(q, p, vol, None, 1e-3)
            coef = fit.coef.detach().requires_grad_()
            row(vol, K, "tps_flow forward", timed(lambda: ops.tps_flow(fit), args.warmup, args.reps, args.rounds), N * K, nd)
            flow = ops.tps_flow(coef, handle=fit)
            row(vol, K, "tps_flow backward",
                timed(lambda: torch.autograd.grad(flow, coef, g, retain_graph=True), args.warmup, args.reps, args.rounds), N * K, nd)
            if not args.no_eager:
                sc = torch.tensor(fit.scale, device=dev)
                qh = fit.ctrl[0] * sc
                c32 = fit.coef[0].detach().float()
                strides = [N // vol[0]] + ([vol[2]] if nd == 3 else []) + [1]

                def grid_fn(i0, i1):
                    idx = torch.arange(i0, i1, device=dev)
                    cols = []
                    for a in range(nd):
                        cols.append((idx // strides[a]) % vol[a] if a else idx // strides[0])
                    return torch.stack(cols, -1).float() * sc

                gflat = g[0].reshape(nd, -1).t().contiguous()
                row(vol, K, "eager forward",
                    timed(lambda: eager_forward(c32, qh, grid_fn, N, K, nd, args.chunk), 1, 1, args.rounds), N * K, nd)
                row(vol, K, "eager backward",
                    timed(lambda: eager_backward(gflat, qh, grid_fn, N, K, nd, args.chunk), 1, 1, args.rounds), N * K, nd)
                ref = eager_forward(c32, qh, grid_fn, N, K, nd, args.chunk).t().reshape(1, nd, *vol)
                lines.append("#   max |tps_flow - eager fp32| = %.3e voxel" % float((ops.tps_flow(fit) - ref).abs().max()))
        if not args.no_eager:
            stride = 8
            ctrl = torch.randn(1, nd, *ops.bspline_control_shape(vol, stride), generator=gen).to(dev).requires_grad_()
            row(vol, "-", "bspline_flow forward", timed(lambda: ops.bspline_flow(ctrl.detach(), vol, stride), args.warmup, args.reps, args.rounds))
            y = ops.bspline_flow(ctrl, vol, stride)
            row(vol, "-", "bspline_flow backward",
                timed(lambda: torch.autograd.grad(y, ctrl, g, retain_graph=True), args.warmup, args.reps, args.rounds))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
