"""GPU box: keypoint detection and sparse matching (dfmir_amd.ops.foerstner_response / local_maxima / keypoint_cost /
keypoint_argmin and infer.keypoint_init, csrc/keypoints.hip) beside an eager torch composition of the same definitions on the
same device -- clamped differences, conv Gaussian (numerator and a ones volume for the renormalised faces), max_pool, a gather of
each keypoint's search region + unfold in chunks of keypoints, argmin -- and beside infer.convex_init on the same pair, at
  3-D  1x1x160x192x224, C = 12 features, K = 2048, the defaults (sigma 1.5, nms 3, search 8 x 2, patch 2)
  2-D  1x1x256x256,     C = 12 features, K = 2048, sigma 1.5, nms 3, search 8 x 2, patch 2

HIP-event timed per call, medians over `--reps` calls after a warm-up (the eager cost, seconds per call, over 2 calls).  Inputs
rotate over a set of images larger than the 256 MiB last-level cache in 3-D.  The sides alternate in one process, three rounds
each, and the median of the rounds' medians is shown.  Every step runs in a child process of its own under its own time limit;
a step that fails or runs out of time ends the run (no retries).  Nothing here is a gate.

    python scripts/bench_keypoints.py [--reps 10] [--out profiles/keypoints_timing.txt]
"""
import argparse
import itertools
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from scripts.bench_invcons import COLD_BYTES, DEV, median_ms  # noqa: E402

CASES = {"3d": dict(shape=(1, 1, 160, 192, 224), C=12, K=2048, sigma=1.5, nms=3, r=8, step=2, patch=2, chunk=8,
                    convex=dict(grid_sp=4, disp_hw=4)),
         "2d": dict(shape=(1, 1, 256, 256), C=12, K=2048, sigma=1.5, nms=3, r=8, step=2, patch=2, chunk=256,
                    convex=dict(grid_sp=2, disp_hw=8))}


def eager_response(I, sigma):
    import torch
    import torch.nn.functional as F
    nd = I.dim() - 2
    g = []
    for a in range(nd):
        n = I.shape[a + 2]
        ip = torch.arange(n, device=I.device).add(1).clamp(max=n - 1)
        im = torch.arange(n, device=I.device).sub(1).clamp(min=0)
        g.append((I.index_select(a + 2, ip) - I.index_select(a + 2, im)) / 2.0)
    prods = torch.cat([g[a] * g[b] for a in range(nd) for b in range(a, nd)], 1)
    r = int(math.ceil(3.0 * sigma))
    w = torch.exp(-torch.arange(-r, r + 1, device=I.device, dtype=torch.float32) ** 2 / (2.0 * sigma * sigma))
    conv = F.conv3d if nd == 3 else F.conv2d
    x = torch.cat([prods, torch.ones_like(I)], 1).movedim(1, 0)             # planes as a batch, the ones volume last
    for a in range(nd):
        shape = [1, 1] + [1] * nd
        shape[a + 2] = 2 * r + 1
        pad = [0] * nd
        pad[a] = r
        x = conv(x, w.view(shape), padding=tuple(pad))
    T = (x[:-1] / x[-1:]).double()
    if nd == 3:
        a, b, c, d, e, f = T
        A00, A11, A22 = d * f - e * e, a * f - c * c, a * d - b * b
        det, tr = a * A00 - b * (b * f - c * e) + c * (b * e - c * d), A00 + A11 + A22
    else:
        a, b, c = T
        det, tr = a * c - b * b, a + c
    return torch.where(tr > 0, det / tr, torch.zeros_like(tr)).float()[None].movedim(0, 1)


def eager_nms(R, radius):
    import torch
    import torch.nn.functional as F
    pool = F.max_pool3d if R.dim() == 5 else F.max_pool2d
    return torch.where((pool(R, 2 * radius + 1, 1, radius) == R) & (R > 0), R, torch.zeros_like(R))      # ties aside


def eager_cost(fix, mov, pts, r, step, patch, chunk):
    import torch
    import torch.nn.functional as F
    nd = fix.dim() - 2
    C = fix.shape[1]
    R0, pw, n = r * step + patch, 2 * patch + 1, 2 * r + 1
    pf, pm = F.pad(fix[0], (R0, R0) * nd), F.pad(mov[0], (R0, R0) * nd)
    q = torch.round(pts[0]).long()
    ar_f = torch.arange(pw, device=fix.device) + (R0 - patch)
    ar_m = torch.arange(2 * R0 + 1, device=fix.device)
    out = []
    for k0 in range(0, q.shape[0], chunk):
        qc = q[k0:k0 + chunk]

        def gather(vol, ar):
            idx = [(qc[:, a, None] + ar[None]) for a in range(nd)]          # [kc, E] per axis
            if nd == 3:
                return vol[:, idx[0][:, :, None, None], idx[1][:, None, :, None], idx[2][:, None, None, :]]
            return vol[:, idx[0][:, :, None], idx[1][:, None, :]]
        fp, reg = gather(pf, ar_f), gather(pm, ar_m)                         # [C, kc, pw..], [C, kc, E..]
        for a in range(nd):
            reg = reg.unfold(2 + a, pw, 1)
        reg = reg[(slice(None), slice(None)) + (slice(None, None, step),) * nd]
        fp = fp.reshape(fp.shape[:2] + (1,) * nd + fp.shape[2:])
        d = (fp - reg).square().sum(tuple(range(2 + nd, 2 + 2 * nd))).sum(0)
        out.append(d.reshape(d.shape[0], -1) / (C * pw ** nd))
    return torch.cat(out)[None]


def eager_argmin(cost, r, step, nd, prior, coeff):
    import torch
    d = torch.tensor(list(itertools.product(range(-r, r + 1), repeat=nd)), dtype=torch.float32, device=cost.device) * step
    idx = (cost + coeff * (d[None, None] - prior[:, :, None]).square().sum(-1)).argmin(2)
    return idx, d[idx]


def _rounds(sides, measure, rounds=3):
    acc = {tag: [] for tag in sides}
    for _ in range(rounds):
        for tag, fn in sides.items():
            acc[tag].append(measure[tag](fn) if isinstance(measure, dict) else measure(fn))
    return {tag: {"ms": round(statistics.median(v), 4), "rounds": [round(x, 4) for x in v]} for tag, v in acc.items()}


def step_case(name, reps):
    import torch
    import torch.nn.functional as F
    from dfmir_amd import infer, ops
    P = CASES[name]
    shape, C, K, r, step, patch = P["shape"], P["C"], P["K"], P["r"], P["step"], P["patch"]
    nd = len(shape) - 2
    vol = shape[2:]
    gen = torch.Generator(device=DEV).manual_seed(3)
    reps = max(3, reps)
    n = min(8, max(2, -(-COLD_BYTES // (4 * math.prod(shape))) // 4))       # images: with their six product planes a cold set
    res = {}
    with torch.no_grad():
        def smooth(*s):
            low = [max(2, v // 4) for v in s[2:]]
            return F.interpolate(torch.rand(*s[:2], *low, device=DEV, generator=gen), size=s[2:],
                                 mode='trilinear' if nd == 3 else 'bilinear', align_corners=True).contiguous()
        imgs = [smooth(*shape) + 0.05 * torch.rand(*shape, device=DEV, generator=gen) for _ in range(n)]
        m = lambda fn: median_ms(lambda i: fn(i % n), reps)
        res["response"] = _rounds({"hip": lambda i: ops.foerstner_response(imgs[i], P["sigma"]),
                                   "eager": lambda i: eager_response(imgs[i], P["sigma"])}, m)
        a, b = ops.foerstner_response(imgs[0], P["sigma"]), eager_response(imgs[0], P["sigma"])
        res["response"]["check"] = float((a - b).abs().max() / b.abs().max())
        Rs = [ops.foerstner_response(t, P["sigma"]) for t in imgs]
        res["nms"] = _rounds({"hip": lambda i: ops.local_maxima(Rs[i], P["nms"]), "eager": lambda i: eager_nms(Rs[i], P["nms"])}, m)
        res["nms"]["equal"] = float((ops.local_maxima(Rs[0], P["nms"]) == eager_nms(Rs[0], P["nms"])).float().mean())
        pts = [ops.select_keypoints(ops.local_maxima(t, P["nms"]), K)[0] for t in Rs]
        res["found"] = int(torch.isfinite(pts[0]).all(-1).sum())
        peaks = [ops.local_maxima(t, P["nms"]) for t in Rs]
        res["select"] = _rounds({"torch": lambda i: ops.select_keypoints(peaks[i], K)}, m)
        del Rs, peaks
        fshape = (1, C) + tuple(vol)
        nf = 2
        feats = [(torch.rand(*fshape, device=DEV, generator=gen), torch.rand(*fshape, device=DEV, generator=gen)) for _ in range(nf)]
        slow = lambda fn: median_ms(lambda i: fn(i % nf), 2, warm=1)
        res["cost"] = _rounds({"hip": lambda i: ops.keypoint_cost(feats[i % nf][0], feats[i % nf][1], pts[i % n], r, step, patch),
                               "eager": lambda i: eager_cost(feats[i][0], feats[i][1], torch.nan_to_num(pts[i % n]), r, step, patch,
                                                             P["chunk"])},
                              {"hip": m, "eager": slow}, rounds=2)
        c0 = ops.keypoint_cost(feats[0][0], feats[0][1], pts[0], r, step, patch)
        c1 = eager_cost(feats[0][0], feats[0][1], torch.nan_to_num(pts[0]), r, step, patch, P["chunk"])
        ok = torch.isfinite(c0)
        res["cost"]["check"] = float((c0 - c1)[ok].abs().max() / c1[ok].abs().max())
        res["cost"]["products"] = C * (2 * patch + 1) ** nd * (2 * r + 1) ** nd
        prior = torch.rand(1, K, nd, device=DEV, generator=gen) * 8 - 4
        cz = torch.nan_to_num(c0, nan=1e30)
        res["argmin"] = _rounds({"hip": lambda i: ops.keypoint_argmin(c0, r, step, prior, 0.1),
                                 "eager": lambda i: eager_argmin(cz, r, step, nd, prior, 0.1)}, m)
        res["argmin"]["equal"] = float((ops.keypoint_argmin(cz, r, step, prior, 0.1)[0]
                                        == eager_argmin(cz, r, step, nd, prior, 0.1)[0]).float().mean())
        del c0, c1, cz
        res["init"] = _rounds({"keypoint_init": lambda i: infer.keypoint_init(imgs[i], imgs[(i + 1) % n], features=feats[i % nf],
                                                                            num_keypoints=K, sigma=P["sigma"], nms_radius=P["nms"],
                                                                            search_radius=r, search_step=step, patch=patch),
                               "convex_init": lambda i: infer.convex_init(imgs[i], imgs[(i + 1) % n], features=feats[i % nf],
                                                                        **P["convex"])}, m)
    return res


def step_bench(_, reps):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                         capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("bench.py ended with status %d: %s" % (out.returncode, out.stderr[-2000:]))
    return {"line": [l for l in out.stdout.splitlines() if l.startswith("{")][-1]}


STEPS = [("case", "3d", 500), ("case", "2d", 300), ("bench", "default", 500)]


def report(res, reps):
    L = ["Keypoint detection and sparse matching (ops.foerstner_response / local_maxima / select_keypoints / keypoint_cost / "
         "keypoint_argmin,", "infer.keypoint_init; dfmir_amd/csrc/keypoints.hip) on one MI355X:",
         "output of `python scripts/bench_keypoints.py --reps %d` (HIP events around whole calls, medians after a warm-up, fp32; the"
         % reps,
         "sides alternate, the median of the rounds' medians is shown; every step in a child process of its own).  `eager` = the",
         "torch composition on the same device: clamped differences + conv Gaussian (with a ones volume for the renormalised faces),",
         "max_pool (ties aside), a gather of each keypoint's search region + unfold in chunks of keypoints, argmin.  Nothing here is",
         "a gate.  The cost kernel has no unstaged variant to compare with: none was built.", ""]
    for name, P in CASES.items():
        c = res["case " + name]
        L.append("%s  C = %d  K = %d (found %d)  sigma %g  nms %d  search %d x %d  patch %d   (%d products per keypoint)"
                 % ("x".join(map(str, P["shape"])), P["C"], P["K"], c["found"], P["sigma"], P["nms"], P["r"], P["step"],
                    P["patch"], c["cost"]["products"]))
        L.append("  %-16s %12s %12s %9s" % ("", "HIP ms", "eager ms", "eager/HIP"))
        for key in ("response", "nms", "cost", "argmin"):
            h, e = c[key]["hip"], c[key]["eager"]
            L.append("  %-16s %12.4f %12.4f %8.2fx   rounds %s / %s%s" % (key, h["ms"], e["ms"], e["ms"] / h["ms"], h["rounds"],
                     e["rounds"], "   SLOWER THAN THE EAGER COMPOSITION" if h["ms"] >= e["ms"] else ""))
        L.append("  %-16s %12.4f   (plain torch on ops.local_maxima's output: a stable sort of the whole volume)" % ("select_keypoints", c["select"]["torch"]["ms"]))
        L.append("  response against eager %.2e (max-abs over max); nms equal to max_pool at %.6f of the voxels; cost against eager "
                 "%.2e; argmin picks equal at %.4f" % (c["response"]["check"], c["nms"]["equal"], c["cost"]["check"],
                                                      c["argmin"]["equal"]))
        k, v = c["init"]["keypoint_init"], c["init"]["convex_init"]
        L.append("  keypoint_init %.3f ms (features given; 7 thin-plate fits with a host sync each, rounds %s) against convex_init(%s) "
                 "%.3f ms (rounds %s)" % (k["ms"], k["rounds"], ", ".join("%s=%d" % kv for kv in P["convex"].items()), v["ms"],
                                          v["rounds"]))
        L.append("")
    L.append("python bench.py --gpus 1 --steps 20 --warmup 5 (unchanged; the default step runs none of the new code):")
    L.append(res["bench default"]["line"])
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=2, default=None, help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    fns = {"case": step_case, "bench": step_bench}
    if args.step:
        kind, arg = args.step
        print("RESULT " + json.dumps(fns[kind](arg, args.reps)), flush=True)
        return 0
    res = {}
    for kind, arg, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
               "--step", kind, arg]
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:
            print("step %s %s ended with status %d; stopping\n%s" % (kind, arg, out.returncode, out.stderr[-3000:]), flush=True)
            return 1
        line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1]
        res[kind + " " + arg] = json.loads(line[7:])
        print("%-6s %-10s %s" % (kind, arg, json.dumps(res[kind + " " + arg])), flush=True)
    text = report(res, args.reps)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
