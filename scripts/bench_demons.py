"""GPU box: the demons solver (dfmir_amd/csrc/gauss.hip, demons.hip) at 160x192x224, in one process:

  (a) ops.gaussian_smooth of a 3-channel field at sigma 1 and 2.5 beside the eager composition -- per axis F.conv3d with a
      (2 r + 1)-tap kernel and zero padding, divided by the (precomputed) same conv of ones -- the two alternating, with the
      achieved fraction of 8 TB/s on the algorithmic bytes (one read plus one write of the tensor);
  (b) ops.demons_force on 12-channel features beside ops.warp_ssd's forward alone and its forward plus backward, on the same
      packed features and flows, with the fraction of 8 TB/s on the bytes a pass needs (packed M, F and the flow read once, d
      written once);
  (c) one iteration of infer.demons_flow (levels=(1,), the defaults otherwise) beside one iteration of infer.refine_flow at
      grid_downsize=1, each as (call with 3 iterations - call with 0 iterations) / 3 on the same 12-channel feature pair.

HIP-event timed per call, medians over `--reps` calls after a warm-up, over a rotating set of inputs whose total exceeds the
256 MiB last-level cache several times (cold buffers); A and B alternate inside the one process, three rounds each.

    python scripts/bench_demons.py [--reps 20] [--out profiles/demons_timing.txt]
"""
import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DEV = "cuda"
VOL = (160, 192, 224)
HBM = 8.0e12


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


def alternate(fns, reps, rounds=3):
    """{tag: (median of the rounds' medians, the rounds)} with the candidates taking turns."""
    acc = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            acc[k].append(median_ms(fn, reps))
    return {k: (statistics.median(v), v) for k, v in acc.items()}


def eager_gauss(sigma, vol):
    """x -> the per-axis F.conv3d composition with its division, the denominators formed once."""
    import torch
    import torch.nn.functional as F
    r = int(math.ceil(3.0 * sigma))
    w = torch.tensor([math.exp(-k * k / (2.0 * sigma * sigma)) for k in range(-r, r + 1)], dtype=torch.float64).float().to(DEV)
    taps, dens = [], []
    for a in range(3):
        shape = [1, 1, 1, 1, 1]
        shape[2 + a] = 2 * r + 1
        pad = [0, 0, 0]
        pad[a] = r
        k = w.reshape(shape)
        ones = [1, 1, 1, 1, 1]
        ones[2 + a] = vol[a]
        taps.append((k, tuple(pad)))
        dens.append(F.conv3d(torch.ones(ones, device=DEV), k, padding=tuple(pad)))

    def run(x):
        B, Cn = x.shape[:2]
        y = x.reshape(B * Cn, 1, *vol)
        for (k, pad), den in zip(taps, dens):
            y = F.conv3d(y, k, padding=pad) / den
        return y.reshape(x.shape)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "demons_timing.txt"))
    args = ap.parse_args()
    import torch
    from dfmir_amd import infer, ops
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    S = math.prod(VOL)
    g = torch.Generator(device=DEV).manual_seed(1)
    emit("the demons solver on %s at %s (scripts/bench_demons.py --reps %d)" % (torch.cuda.get_device_name(0), "x".join(map(str, VOL)), args.reps))
    emit("medians of 3 alternating rounds x %d calls, HIP events; every input comes from a rotating set larger than the 256 MiB cache" % args.reps)
    emit()

    fields = [torch.rand(1, 3, *VOL, device=DEV, generator=g) * 2 - 1 for _ in range(8)]          # 8 x 83 MB
    n = len(fields)
    emit("(a) ops.gaussian_smooth, a field 1x3x%s (%.1f MB; algorithmic bytes = one read + one write)" % ("x".join(map(str, VOL)), 12e-6 * S))
    for sigma in (1.0, 2.5):
        eager = eager_gauss(sigma, VOL)
        res = alternate({"ops.gaussian_smooth": lambda i: ops.gaussian_smooth(fields[i % n], sigma),
                         "eager F.conv3d per axis / ones": lambda i: eager(fields[i % n])}, args.reps)
        a, b = ops.gaussian_smooth(fields[0], sigma), eager(fields[0])
        for tag, (t, rounds) in res.items():
            emit("    sigma %-4g %-32s %8.4f ms   %.3f of 8 TB/s   rounds %s"
                 % (sigma, tag, t, 2 * 12.0 * S / (t * 1e-3) / HBM, ["%.4f" % v for v in rounds]))
        emit("    sigma %-4g eager / kernel = %.2f x;  kernel vs eager, max-abs over max: %.2e"
             % (sigma, res["eager F.conv3d per axis / ones"][0] / res["ops.gaussian_smooth"][0], float((a - b).abs().max() / b.abs().max())))
        del a, b
    del fields
    torch.cuda.empty_cache()
    emit()

    Cn = 12
    sets = []
    for i in range(2):                                                                            # 2 x (330 + 330 + 83) MB
        M, Fx = torch.rand(1, Cn, *VOL, device=DEV, generator=g), torch.rand(1, Cn, *VOL, device=DEV, generator=g)
        phi = (torch.rand(1, 3, *VOL, device=DEV, generator=g) * 2 - 1) * 1.5
        sets.append((ops.pack_features(M), Fx, phi, phi.clone().requires_grad_()))
    n = len(sets)
    nbytes = 4.0 * S * (Cn + Cn + 3 + 3)
    emit("(b) ops.demons_force, features 1x%dx%s, flows of up to 1.5 voxels (bytes of a pass: packed M, F, flow in, d out = %.0f MB)"
         % (Cn, "x".join(map(str, VOL)), nbytes * 1e-6))
    res = alternate({"ops.demons_force": lambda i: ops.demons_force(sets[i % n][0], sets[i % n][1], sets[i % n][2]),
                     "ops.warp_ssd forward": lambda i: ops.warp_ssd(sets[i % n][0], sets[i % n][1], sets[i % n][2]),
                     "ops.warp_ssd forward + backward": lambda i: torch.autograd.grad(
                         ops.warp_ssd(sets[i % n][0], sets[i % n][1], sets[i % n][3]), sets[i % n][3])}, args.reps)
    for tag, (t, rounds) in res.items():
        emit("    %-34s %8.4f ms   %.3f of 8 TB/s   rounds %s" % (tag, t, nbytes / (t * 1e-3) / HBM, ["%.4f" % v for v in rounds]))
    emit("    demons_force / warp_ssd forward = %.2f x,  / forward + backward = %.2f x"
         % (res["ops.demons_force"][0] / res["ops.warp_ssd forward"][0], res["ops.demons_force"][0] / res["ops.warp_ssd forward + backward"][0]))
    Ld, Lw = ops.demons_force(*sets[0][:3])[1], ops.warp_ssd(*sets[0][:3])
    emit("    L of demons_force vs warp_ssd, relative: %.2e" % float((Ld - Lw).abs() / Lw))
    emit()

    emit("(c) one iteration on the same %d-channel feature pair, (call with 3 iterations - call with 0) / 3" % Cn)
    feats = [(sets[i][0].planar, sets[i][1]) for i in range(n)]
    img = feats[0][0][:, :1].contiguous()
    r = max(3, args.reps // 4)
    dm = lambda it: (lambda i: infer.demons_flow(img, img, features=feats[i % n], levels=(1,), iters=it))
    rf = lambda it: (lambda i: infer.refine_flow(img, img, features=feats[i % n], lam=0.1, lr=0.1, grid_downsize=1, iters=it))
    res = alternate({"demons_flow iters=3": dm(3), "demons_flow iters=0": dm(0), "refine_flow iters=3": rf(3), "refine_flow iters=0": rf(0)}, r)
    for tag, (t, rounds) in res.items():
        emit("    %-34s %8.4f ms   rounds %s" % (tag, t, ["%.4f" % v for v in rounds]))
    t_dm = (res["demons_flow iters=3"][0] - res["demons_flow iters=0"][0]) / 3
    t_rf = (res["refine_flow iters=3"][0] - res["refine_flow iters=0"][0]) / 3
    emit("    one demons_flow iteration (force, fluid Gaussian, compose, diffusion Gaussian)   %8.4f ms" % t_dm)
    emit("    one refine_flow iteration (resize, warp_ssd, diffusion, backward, Adam)          %8.4f ms   refine / demons = %.2f x" % (t_rf, t_rf / t_dm))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
