"""GPU box: affine pre-alignment (dfmir_amd/csrc/affine.hip) at 1x12x160x192x224 and 16x4x256x256, the shapes of
scripts/bench_refine.py, in one process:

  (a) value + gradient: ops.affine_ssd + backward beside the composition the shipped pieces give once ops.affine_flow exists --
      affine_flow -> warp_ssd -> backward -> affine_flow's adjoint -- on the same inputs, the two alternating;
  (b) the full system ops.affine_ssd_system beside ops.warp_ssd's forward + flow gradient at the same shape (what the extra
      sums cost; there is no shipped equivalent) and, at the 2-D shape, beside an eager torch composition of H from per-voxel
      Jacobians (the corners gathered with explicit indices, J = dM (x) q, H = J^T J by einsum);
  (c) infer.affine_init with its defaults at the 3-D shape on MIND-sized feature pairs: the whole call, each level alone, and
      the host time of a call (taken before the device is waited for: a call that synced would show the device time there).

HIP-event timed per call, medians over `--reps` calls after a warm-up, over a rotating set of inputs (every feature tensor of
the 3-D shape is larger than the 256 MiB last-level cache; the two sets of the 2-D shape fit into it, so its figures are
warm-cache ones).  The thetas are registration-like: 3 degrees, 3 %, 2 voxels.  The
register and occupancy figures of af_sys_k come from `hipcc -Rpass-analysis=kernel-resource-usage` on affine.hip (--resources
FILE takes a saved copy of that output).

    python scripts/bench_affine.py [--reps 20] [--out profiles/affine_timing.txt]
"""
import argparse
import math
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

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


def resource_usage(saved):
    """[(kernel, VGPRs, scratch bytes, waves/SIMD, LDS bytes)] of the af_sys_k instantiations."""
    if saved:
        text = open(saved).read()
    else:
        csrc = os.path.join(REPO, "dfmir_amd", "csrc")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
               "-Rpass-analysis=kernel-resource-usage", "-c", "affine.hip", "-o", os.devnull]
        text = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True).stderr
    rows = []
    for m in re.finditer(r"Function Name: (\S*af_sys_kILi(\d)ELb(\d)\S*)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        body = m.group(4)
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", body).group(1))
        rows.append(("af_sys_k<%s-D, %s>" % (m.group(2), "full" if m.group(3) == "1" else "gradient"), get(" VGPRs"),
                     get("ScratchSize [bytes/lane]"), get("Occupancy [waves/SIMD]"), int(m.group(5))))
    return rows


def make_inputs(shape):
    import torch
    g = torch.Generator(device=DEV).manual_seed(1)
    B, nd = shape[0], len(shape) - 2
    out = []
    for i in range(SETS):
        a = math.radians(3.0) * (1 if i else -1)
        th = torch.eye(nd, nd + 1)
        th[nd - 2, nd - 2], th[nd - 2, nd - 1], th[nd - 1, nd - 2], th[nd - 1, nd - 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
        th[:, :nd] *= 1.03
        th[:, nd] = torch.tensor([1.5, -2.0, 0.75][:nd])
        out.append((torch.rand(*shape, device=DEV, generator=g), torch.rand(*shape, device=DEV, generator=g),
                    th.repeat(B, 1, 1).to(DEV).requires_grad_()))
    return out


def eager_system(M, Fx, theta):
    """(L_b, g, H) by eager torch from per-voxel Jacobians: the four corners gathered with explicit indices, the interpolant
    and its corner differences, J = dM (x) q, g = k J^T e, H = k J^T J by einsum."""
    import torch
    B, Cn, Hh, W = M.shape
    ys, xs = torch.meshgrid(torch.arange(Hh, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32),
                            indexing='ij')
    q = torch.stack([ys - (Hh - 1) / 2.0, xs - (W - 1) / 2.0, torch.ones_like(ys)], 0)                  # [3,H,W]
    id3 = torch.eye(2, 3, device=DEV)[None]
    y = torch.einsum('baj,jhw->bahw', theta - id3, q) + torch.stack([ys, xs], 0)[None]
    i0 = torch.floor(y)
    w1 = y - i0
    i0 = i0.long()
    Mf = M.reshape(B, Cn, Hh * W)

    def corner(dy, dx):
        iy, ix = i0[:, 0] + dy, i0[:, 1] + dx
        valid = (iy >= 0) & (iy < Hh) & (ix >= 0) & (ix < W)
        idx = (iy.clamp(0, Hh - 1) * W + ix.clamp(0, W - 1)).reshape(B, 1, -1).expand(B, Cn, -1)
        return torch.gather(Mf, 2, idx).reshape(B, Cn, Hh, W) * valid[:, None]

    v00, v01, v10, v11 = corner(0, 0), corner(0, 1), corner(1, 0), corner(1, 1)
    wy, wx = w1[:, 0:1], w1[:, 1:2]
    e = (1 - wy) * ((1 - wx) * v00 + wx * v01) + wy * ((1 - wx) * v10 + wx * v11) - Fx
    dM = torch.stack([(1 - wx) * (v10 - v00) + wx * (v11 - v01), (1 - wy) * (v01 - v00) + wy * (v11 - v10)], 2)   # [B,C,2,H,W]
    J = (dM[:, :, :, None] * q[None, None, None]).reshape(B, Cn, 6, Hh * W)                           # [B,C,P,S]
    k = 2.0 / (Cn * Hh * W)
    return (e ** 2).mean((1, 2, 3)), k * torch.einsum('bcps,bcs->bp', J, e.reshape(B, Cn, -1)), k * torch.einsum('bcps,bcrs->bpr', J, J)


def bench_shape(name, reps, emit):
    import torch
    from dfmir_amd import infer, ops
    shape = SHAPES[name]
    vol = shape[2:]
    sets = make_inputs(shape)
    handles = [ops.pack_features(M) for M, _, _ in sets]
    n = len(sets)

    def fused(i):
        _, Fx, th = sets[i % n]
        return torch.autograd.grad(ops.affine_ssd(handles[i % n], Fx, th), th)

    def composed(i):
        _, Fx, th = sets[i % n]
        return torch.autograd.grad(ops.warp_ssd(handles[i % n], Fx, ops.affine_flow(th, vol)), th)

    def system(i):
        _, Fx, th = sets[i % n]
        return ops.affine_ssd_system(handles[i % n], Fx, th.detach())

    def warp_ssd_grad(i):
        _, Fx, th = sets[i % n]
        phi = flows[i % n]
        return torch.autograd.grad(ops.warp_ssd(handles[i % n], Fx, phi), phi)

    flows = [ops.affine_flow(th.detach(), vol).requires_grad_() for _, _, th in sets]
    acc = {"affine_ssd + backward": [], "affine_flow -> warp_ssd -> backward -> adjoint": []}
    for _ in range(3):                                   # the two alternate, three rounds each
        acc["affine_ssd + backward"].append(median_ms(fused, reps))
        acc["affine_flow -> warp_ssd -> backward -> adjoint"].append(median_ms(composed, reps))
    a, b = fused(0)[0], composed(0)[0]
    emit("%s  (B x C x vol; %d input sets, medians of 3 rounds x %d calls)" % (name, n, reps))
    emit("  (a) value + gradient")
    for tag, v in acc.items():
        emit("      %-48s %8.4f ms   rounds %s" % (tag, statistics.median(v), ["%.4f" % x for x in v]))
    emit("      composition / fused = %.2f x;  dtheta fused vs composition, max-abs over max: %.2e"
         % (statistics.median(acc["affine_flow -> warp_ssd -> backward -> adjoint"]) / statistics.median(acc["affine_ssd + backward"]),
            float((a - b).abs().max() / b.abs().max())))
    emit("  (b) full system")
    t_sys, t_ws = median_ms(system, reps), median_ms(warp_ssd_grad, reps)
    emit("      %-48s %8.4f ms" % ("affine_ssd_system (L_b, g, H)", t_sys))
    emit("      %-48s %8.4f ms   system / warp_ssd = %.2f x" % ("warp_ssd forward + dflow", t_ws, t_sys / t_ws))
    if len(vol) == 2:
        try:
            t_eager = median_ms(lambda i: eager_system(sets[i % n][0], sets[i % n][1], sets[i % n][2].detach()), max(3, reps // 4), warm=1)
            Hk, He = system(0)[2], eager_system(sets[0][0], sets[0][1], sets[0][2].detach())[2]
            emit("      %-48s %8.4f ms   eager / system = %.1f x   (H eager vs kernel, max-abs over max: %.1e)"
                 % ("eager torch, per-voxel Jacobians", t_eager, t_eager / t_sys, float((Hk - He.double()).abs().max() / Hk.abs().max())))
        except torch.cuda.OutOfMemoryError:
            emit("      eager torch, per-voxel Jacobians: does not fit in memory")
    if len(vol) == 3:
        emit("  (c) infer.affine_init, defaults (levels (4, 2, 1), 10 evaluations each), a pair of %d-channel feature tensors" % shape[1])
        M, Fx, _ = sets[0]
        img = M[:, :1].contiguous()
        r = max(3, reps // 4)
        call = lambda **kw: median_ms(lambda i: infer.affine_init(img, img, features=(sets[i % n][0], sets[i % n][1]), **kw), r, warm=1)
        emit("      %-48s %8.4f ms" % ("whole call", call()))
        emit("      %-48s %8.4f ms" % ("iters=0 (the final affine_flow + warp alone)", call(iters=0)))
        for s in (4, 2, 1):
            emit("      %-48s %8.4f ms" % ("levels=(%d,) alone" % s, call(levels=(s,))))
        torch.cuda.synchronize()
        host = []
        for i in range(r):
            t0 = time.perf_counter()
            out = infer.affine_init(img, img, features=(M, Fx))
            host.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
        emit("      %-48s %8.4f ms   (returned before the device was waited for)" % ("host time of a call", statistics.median(host)))
        del out
    emit("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "affine_timing.txt"))
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    import torch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("affine pre-alignment on %s (scripts/bench_affine.py --reps %d)" % (torch.cuda.get_device_name(0), args.reps))
    emit("")
    emit("af_sys_k, hipcc -Rpass-analysis=kernel-resource-usage (gfx950, 256 threads per workgroup):")
    for k, vg, sc, occ, lds in resource_usage(args.resources):
        emit("  %-28s %3d VGPRs, %d bytes of scratch per lane, %d waves/SIMD, %5d bytes of LDS per workgroup" % (k, vg, sc, occ, lds))
    emit("")
    for name in SHAPES:
        bench_shape(name, args.reps, emit)
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
