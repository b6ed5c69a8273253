"""GPU box: the discrete displacement search (dfmir_amd.ops.pool_features / ssd_cost_volume / cost_argmin / box_smooth_flow and
infer.convex_init, csrc/dsearch.hip) beside an eager torch composition on the same device -- avg_pool, pad and a slicing loop
over the displacements, argmin, avg_pool(3, 1, 1, count_include_pad=False) -- at
  3-D  1x12x160x192x224 (the MIND channel count), g = 4, r = 3 and g = 2, r = 2
  2-D  16x4x256x256, g = 2, r = 4
per kernel and for the whole convex_init (on a given feature pair: the descriptors are the same work on both sides).

HIP-event timed per call, medians over `--reps` calls after a warm-up.  Inputs rotate over a set of at least 640 MiB, larger
than the 256 MiB last-level cache, and the outputs of the last calls are kept alive in a ring of the same size, so the
allocator hands every call a block that is not cache-resident: the cost volume is neither read nor written through the
cache.  The sides alternate in one process, three rounds each, and the median of the rounds' medians is shown.  For the cost
kernel the fraction of the HBM write roofline is 4 B K S bytes / time / 8 TB/s.  Every step runs in a child process of its
own under its own time limit; a step that fails or runs out of time ends the run (no retries).  Nothing here is a gate.

    python scripts/bench_dsearch.py [--reps 10] [--out profiles/dsearch_timing.txt]
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
from scripts.bench_invcons import COLD_BYTES, DEV, HBM_TBS, median_ms  # noqa: E402

CASES = {"3d_g4_r3": ((1, 12, 160, 192, 224), 4, 3), "3d_g2_r2": ((1, 12, 160, 192, 224), 2, 2),
         "2d_g2_r4": ((16, 4, 256, 256), 2, 4)}
COEFFS = (0.003, 0.01, 0.03, 0.1, 0.3, 1.0)


def _mesh(nd, r):
    import torch
    return torch.tensor(list(itertools.product(range(-r, r + 1), repeat=nd)), dtype=torch.float32, device=DEV)


def eager_pool(M, g):
    import torch.nn.functional as F
    return (F.avg_pool3d if M.dim() == 5 else F.avg_pool2d)(M, g)


def eager_cost(fix, mov, r):
    import torch
    import torch.nn.functional as F
    nd = fix.dim() - 2
    vol = fix.shape[2:]
    pm = F.pad(mov, (r, r) * nd)
    out = []
    for d in itertools.product(range(-r, r + 1), repeat=nd):
        sl = (slice(None), slice(None)) + tuple(slice(r + d[a], r + d[a] + vol[a]) for a in range(nd))
        out.append(((fix - pm[sl]) ** 2).mean(1))
    return torch.stack(out, 1)


def eager_argmin(cost, r, soft=None, coeff=0.0):
    nd = cost.dim() - 2
    m = _mesh(nd, r)
    J = cost
    if soft is not None:
        J = cost + coeff * ((m.reshape((1, -1, nd) + (1,) * nd) - soft[:, None]) ** 2).sum(2)
    idx = J.argmin(1)
    return idx, m[idx].movedim(-1, 1).contiguous()


def eager_smooth(disp):
    import torch.nn.functional as F
    return (F.avg_pool3d if disp.dim() == 5 else F.avg_pool2d)(disp, 3, 1, 1, count_include_pad=False)


def eager_convex(Mm, Mf, g, r, coeffs=COEFFS):
    import torch.nn.functional as F
    cost = eager_cost(eager_pool(Mf, g), eager_pool(Mm, g), r)
    idx, disp = eager_argmin(cost, r)
    soft = eager_smooth(disp)
    for c in coeffs:
        idx, disp = eager_argmin(cost, r, soft, c)
        soft = eager_smooth(disp)
    nd = Mm.dim() - 2
    return F.interpolate(soft, size=Mm.shape[2:], mode='trilinear' if nd == 3 else 'bilinear', align_corners=True) * g, soft, idx


def _rounds(sides, measure, rounds=3):
    acc = {tag: [] for tag in sides}
    for _ in range(rounds):
        for tag, fn in sides.items():
            acc[tag].append(measure(fn))
    return {tag: {"ms": round(statistics.median(v), 4), "rounds": [round(x, 4) for x in v]} for tag, v in acc.items()}


def step_case(name, reps):
    import torch
    from dfmir_amd import infer, ops
    shape, g, r = CASES[name]
    nd = len(shape) - 2
    gen = torch.Generator(device=DEV).manual_seed(3)
    rnd = lambda *s: torch.rand(*s, device=DEV, generator=gen) * 2.0 - 1.0
    sp = tuple(n // g for n in shape[2:])
    B, K, S = shape[0], (2 * r + 1) ** nd, math.prod(sp)
    res = {"coarse": list(sp), "K": K, "cost_bytes": 4 * B * K * S}
    ring = lambda nbytes: max(2, -(-COLD_BYTES // nbytes))
    reps = max(3, reps)

    def timed(n_in, n_out):
        """measure(fn): fn(i) over n_in rotating inputs, the last n_out results kept alive"""
        keep = [None] * n_out
        return lambda fn: median_ms(lambda i: keep.__setitem__(i % n_out, fn(i % n_in)), reps)

    with torch.no_grad():
        # pooling: rotating full-resolution features
        n = ring(4 * math.prod(shape))
        feats = [rnd(*shape) for _ in range(n)]
        m = timed(n, 2)
        res["pool"] = _rounds({"hip": lambda i: ops.pool_features(feats[i], g), "eager": lambda i: eager_pool(feats[i], g)}, m)
        # cost volume: rotating pooled pairs (small), outputs kept alive in a ring larger than the cache
        pooled = [(ops.pool_features(feats[i], g), ops.pool_features(feats[(i + 1) % n], g)) for i in range(n)]
        del feats
        nc = ring(res["cost_bytes"]) + 1
        m = timed(n, nc)
        res["cost"] = _rounds({"hip": lambda i: ops.ssd_cost_volume(pooled[i][0], pooled[i][1], r),
                               "eager": lambda i: eager_cost(pooled[i][0], pooled[i][1], r)}, m)
        res["cost"]["write_roofline"] = round(res["cost_bytes"] / (res["cost"]["hip"]["ms"] * 1e-3) / (HBM_TBS * 1e12), 4)
        # the cost kernel alone: packed inputs made beforehand, outputs of a preallocated ring
        from dfmir_amd._lib import check, lib
        geom = ops._features_geom(pooled[0][0], "bench")
        pk = [tuple(ops._dsearch_pool(t, geom, 1, False, True)[1] for t in pr) for pr in pooled]
        outs = [torch.empty((B, K) + sp, device=DEV) for _ in range(nc)]
        D, H, W = (1,) * (3 - nd) + sp
        res["cost"]["kernel_ms"] = round(statistics.median(median_ms(lambda i: check(lib().dfmir_dsearch_cost(
            nd, ops._p(pk[i % n][0]), ops._p(pk[i % n][1]), ops._p(outs[i % nc]), B, shape[1], D, H, W, r, ops._st())), reps)
            for _ in range(3)), 4)
        res["cost"]["kernel_write_roofline"] = round(res["cost_bytes"] / (res["cost"]["kernel_ms"] * 1e-3) / (HBM_TBS * 1e12), 4)
        del pk, outs
        a, b = ops.ssd_cost_volume(*pooled[0], r), eager_cost(*pooled[0], r)
        res["cost"]["check"] = float((a - b).abs().max() / b.abs().max())
        del a, b
        # argmin: rotating cost volumes and soft fields
        costs = [ops.ssd_cost_volume(pooled[i % n][0], pooled[i % n][1], r) for i in range(nc)]
        softs = [rnd(B, nd, *sp) * r for _ in range(nc)]
        m = timed(nc, 4)
        res["argmin"] = _rounds({"hip": lambda i: ops.cost_argmin(costs[i], r, softs[i], 0.1),
                                 "eager": lambda i: eager_argmin(costs[i], r, softs[i], 0.1)}, m)
        res["argmin"]["read_roofline"] = round(res["cost_bytes"] / (res["argmin"]["hip"]["ms"] * 1e-3) / (HBM_TBS * 1e12), 4)
        res["argmin"]["picks_equal"] = float((ops.cost_argmin(costs[0], r, softs[0], 0.1)[0]
                                              == eager_argmin(costs[0], r, softs[0], 0.1)[0]).float().mean())
        disps = [ops.cost_argmin(costs[i], r)[1] for i in range(nc)]
        res["smooth"] = _rounds({"hip": lambda i: ops.box_smooth_flow(disps[i]), "eager": lambda i: eager_smooth(disps[i])}, m)
        del costs, softs, disps, pooled
        # the whole first stage on a given feature pair
        n = max(2, ring(8 * math.prod(shape)))
        fp = [(rnd(*shape), rnd(*shape)) for _ in range(n)]
        img = torch.zeros((B, 1) + tuple(shape[2:]), device=DEV)
        m = timed(n, 2)
        res["convex_init"] = _rounds({"hip": lambda i: infer.convex_init(img, img, features=fp[i], grid_sp=g, disp_hw=r),
                                      "eager": lambda i: eager_convex(fp[i][0], fp[i][1], g, r)}, m)
        x, y = infer.convex_init(img, img, features=fp[0], grid_sp=g, disp_hw=r), eager_convex(fp[0][0], fp[0][1], g, r)
        res["convex_init"]["idx_equal"] = float((x["idx"] == y[2]).float().mean())
    return res


def step_bench(_, reps):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                         capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("bench.py ended with status %d: %s" % (out.returncode, out.stderr[-2000:]))
    return {"line": [l for l in out.stdout.splitlines() if l.startswith("{")][-1]}


STEPS = [("case", "3d_g4_r3", 500), ("case", "3d_g2_r2", 500), ("case", "2d_g2_r4", 400), ("bench", "default", 600)]


def report(res, reps):
    L = ["Discrete displacement search (ops.pool_features / ssd_cost_volume / cost_argmin / box_smooth_flow, infer.convex_init; "
         "dfmir_amd/csrc/dsearch.hip) on one MI355X:",
         "output of `python scripts/bench_dsearch.py --reps %d` (HIP events around whole calls, medians after a warm-up, fp32; inputs"
         % reps,
         "rotate over at least 640 MiB and the last outputs are kept alive in a ring of that size, so the cost volume is neither",
         "read nor written through the 256 MiB last-level cache; the sides alternate, three rounds each, the median of the rounds'",
         "medians is shown; every step in a child process of its own).  `eager` = the torch composition on the same device: avg_pool,",
         "pad + one slice per displacement, argmin, avg_pool(3, 1, 1, count_include_pad=False).  Nothing here is a gate.", ""]
    for name, (shape, g, r) in CASES.items():
        c = res["case " + name]
        L.append("%s  g = %d  r = %d   coarse %s, K = %d, cost volume %.1f MiB"
                 % ("x".join(map(str, shape)), g, r, "x".join(map(str, c["coarse"])), c["K"], c["cost_bytes"] / 2 ** 20))
        L.append("  %-16s %12s %12s %9s" % ("", "HIP ms", "eager ms", "eager/HIP"))
        for key in ("pool", "cost", "argmin", "smooth", "convex_init"):
            h, e = c[key]["hip"], c[key]["eager"]
            L.append("  %-16s %12.4f %12.4f %8.2fx   rounds %s / %s%s" % (key, h["ms"], e["ms"], e["ms"] / h["ms"], h["rounds"], e["rounds"],
                     "   SLOWER THAN THE EAGER COMPOSITION" if h["ms"] >= e["ms"] else ""))
        L.append("  cost: ssd_cost_volume (packs both sides, then the cost kernel) writes 4 B K S bytes at %.1f %% of the 8 TB/s HBM "
                 "roofline; the cost kernel alone %.4f ms = %.1f %%; against eager %.2e (max-abs over max)"
                 % (100 * c["cost"]["write_roofline"], c["cost"]["kernel_ms"], 100 * c["cost"]["kernel_write_roofline"],
                    c["cost"]["check"]))
        L.append("  argmin: reads the cost volume at %.1f %% of 8 TB/s; picks equal to the eager argmin at %.4f of the voxels; "
                 "convex_init idx equal at %.4f" % (100 * c["argmin"]["read_roofline"], c["argmin"]["picks_equal"],
                                                    c["convex_init"]["idx_equal"]))
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
