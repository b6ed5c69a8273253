"""GPU box: the cubic B-spline expansion (dfmir_amd.ops.bspline_flow, csrc/bspline.hip) at 1x3x160x192x224 and 16x2x256x256,
control spacing 4, forward and backward, beside
  (a) eager    the depthwise conv_transpose{2,3}d with the separable 16-tap-per-axis kernel, cropped, and its autograd backward;
  (b) linear   ops.resize_linear from the vol // 4 grid to the same output, forward and backward: what refine_flow's loop runs
               with parametrisation='linear' (kernels unchanged by this work);
the forward also as a share of the 8 TB/s HBM peak on the bytes it must move (the field written plus the control grid read);
then 50 iterations of infer.refine_flow at 16x20x24 and 160x192x224 with both parametrisations, grid_downsize 4.

HIP-event timed per call, medians over `--reps` calls after a warm-up.  Every timed call works on its own slot of a rotating
set larger than the 256 MiB last-level cache: the backward reads a cold dy, the forward writes an output block that is kept
alive until the ring comes round (so the allocator cannot hand the same block back).  The sides alternate in one process, three
rounds each, and the median of the rounds' medians is shown.  Every step runs in a child process of its own under its own time
limit; a step that fails or runs out of time ends the run (no retries).  Nothing here is a gate.

    python scripts/bench_bspline.py [--reps 20] [--out profiles/bspline_timing.txt]

Kernel times (the calls above include the launch and the allocation of the output) come from a traced run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_bspline.py --trace 1x3x160x192x224
which runs TRACE_CALLS forward + backward calls of bspline_flow and of resize_linear over the rotating set and nothing else.
"""
import argparse
import json
import math
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from scripts.bench_compose import _rounds  # noqa: E402
from scripts.bench_invcons import COLD_BYTES, DEV, SHAPES, median_ms  # noqa: E402

STRIDE = 4
HBM_PEAK = 8.0e12
REFINE_VOLS = {"16x20x24": (16, 20, 24), "160x192x224": (160, 192, 224)}
REFINE_ITERS = 50
TRACE_CALLS = 20


def eager_weight(nd, channels):
    """[C,1,*(4 s)] fp32: the separable kernel k[(3 - l) s + r] = B_l(r / s) of the conv_transpose form"""
    import torch
    t = torch.arange(STRIDE, dtype=torch.float64) / STRIDE
    B = [(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6]
    k1 = torch.cat([B[3], B[2], B[1], B[0]])
    k = k1
    for a in range(1, nd):
        k = k[..., None] * k1.reshape((1,) * a + (-1,))
    return k[None, None].expand((channels, 1) + tuple(k.shape)).contiguous().float().to(DEV)


def sides_for(shape, which):
    """{tag: (fn(grid) -> [B,C,*vol], shape of the grid)}"""
    import torch.nn.functional as F
    from dfmir_amd import ops
    vol = tuple(shape[2:])
    nd = len(vol)
    m = ops.bspline_control_shape(vol, STRIDE)
    out = {"bspline": (lambda c: ops.bspline_flow(c, vol, STRIDE), m)}
    if which == "eager":
        w = eager_weight(nd, shape[1])
        conv = F.conv_transpose3d if nd == 3 else F.conv_transpose2d

        def eager(c):
            y = conv(c, w, stride=STRIDE, groups=shape[1])
            for a, n in enumerate(vol):
                y = y.narrow(2 + a, 3 * STRIDE, n)
            return y
        out["eager"] = (eager, m)
    else:
        out["linear"] = (lambda c: ops.resize_linear(c, vol), tuple(n // STRIDE for n in vol))
    return out


def step_op(name, reps, which):
    import torch
    shape = SHAPES[name]
    n = max(2, -(-COLD_BYTES // (4 * math.prod(shape))))
    g = torch.Generator(device=DEV).manual_seed(1)
    dys = [torch.rand(*shape, device=DEV, generator=g) * 2 - 1 for _ in range(n)]
    sides = sides_for(shape, which)
    grids = {tag: [(torch.rand(*shape[:2], *m, device=DEV, generator=g) * 2 - 1).requires_grad_() for _ in range(n)]
             for tag, (_, m) in sides.items()}

    def measure(tag):
        fn, cs = sides[tag][0], grids[tag]
        ring = [None] * n

        def fwd(i):
            ring[i % n] = fn(cs[i % n])
        with torch.no_grad():
            f = median_ms(fwd, max(3, reps))
        del ring[:]
        ys = [fn(c) for c in cs]
        b = median_ms(lambda i: torch.autograd.grad(ys[i % n], cs[i % n], dys[i % n], retain_graph=True), max(3, reps))
        return {"fwd_ms": f, "bwd_ms": b}
    res = _rounds({tag: tag for tag in sides}, measure)
    res["slots"] = n
    res["fwd_bytes"] = 4 * (math.prod(shape) + math.prod(shape[:2]) * math.prod(sides["bspline"][1]))
    if which == "eager":
        c = grids["bspline"][0]
        a, b = sides["bspline"][0](c), sides["eager"][0](c)
        ga, gb = torch.autograd.grad(a, c, dys[0])[0], torch.autograd.grad(b, c, dys[0])[0]
        res["check"] = [float((a - b).abs().max() / b.abs().max()), float((ga - gb).abs().max() / gb.abs().max())]
    return res


def step_refine(name, reps, _):
    import torch
    import torch.nn.functional as F
    from dfmir_amd import infer
    torch.manual_seed(0)
    vol = REFINE_VOLS[name]
    blur = lambda x: F.interpolate(F.interpolate(x, scale_factor=0.25, mode='trilinear'), size=vol, mode='trilinear')
    A = blur(torch.rand(1, 1, *vol, device=DEV)).contiguous()
    B = (0.7 * A + 0.3 * blur(torch.rand(1, 1, *vol, device=DEV))).contiguous()
    kw = dict(features='intensity', lam=0.05, lr=0.1, iters=REFINE_ITERS, grid_downsize=STRIDE)
    sides = {p: (lambda p=p: infer.refine_flow(A, B, parametrisation=p, **kw)) for p in ("bspline", "linear")}
    res = _rounds(sides, lambda fn: {"ms_per_iter": median_ms(lambda i: fn(), max(3, reps // 4), warm=1) / REFINE_ITERS})
    hist = {p: fn()["history"].cpu() for p, fn in sides.items()}
    res["similarity"] = {p: [float(h[0, 0]), float(h[-1, 0])] for p, h in hist.items()}
    return res


def trace(name):
    import torch
    shape = SHAPES[name]
    n = max(2, -(-COLD_BYTES // (4 * math.prod(shape))))
    g = torch.Generator(device=DEV).manual_seed(1)
    dys = [torch.rand(*shape, device=DEV, generator=g) * 2 - 1 for _ in range(n)]
    for tag, (fn, m) in sides_for(shape, "op").items():
        cs = [(torch.rand(*shape[:2], *m, device=DEV, generator=g) * 2 - 1).requires_grad_() for _ in range(n)]
        for i in range(TRACE_CALLS):
            torch.autograd.grad(fn(cs[i % n]), cs[i % n], dys[i % n])
    torch.cuda.synchronize()
    return 0


STEPS = [("op", "1x3x160x192x224", 400), ("op", "16x2x256x256", 300), ("refine", "16x20x24", 300),
         ("refine", "160x192x224", 400), ("eager", "16x2x256x256", 400), ("eager", "1x3x160x192x224", 600)]


def report(res, reps):
    L = ["Cubic B-spline expansion (ops.bspline_flow, dfmir_amd/csrc/bspline.hip) on one MI355X, control spacing %d: output of "
         "`python scripts/bench_bspline.py --reps %d`" % (STRIDE, reps),
         "(HIP events around whole calls, medians after a warm-up, fp32; every call works on its own slot of a rotating set larger",
         "than the 256 MiB last-level cache; the sides alternate, three rounds each, the median of the rounds' medians is shown; every",
         "step in a child process of its own).  Nothing here is a gate.", ""]
    for name in SHAPES:
        r, e = res["op " + name], res.get("eager " + name)
        L.append("%s (%d rotating slots)                          forward      backward" % (name, r["slots"]))
        rows = [("bspline_flow (HIP)", r["bspline"]), ("(b) ops.resize_linear from vol // 4", r["linear"])]
        if e:
            rows += [("bspline_flow, beside (a)", e["bspline"]), ("(a) eager conv_transpose + crop", e["eager"])]
        for label, d in rows:
            L.append("  %-38s %9.4f ms %9.4f ms     rounds fwd %s  bwd %s"
                     % (label, d["fwd_ms"], d["bwd_ms"], d["rounds"]["fwd_ms"], d["rounds"]["bwd_ms"]))
        L.append("  %-38s %9.2fx   %9.2fx" % ("(b) / bspline_flow", r["linear"]["fwd_ms"] / r["bspline"]["fwd_ms"],
                                              r["linear"]["bwd_ms"] / r["bspline"]["bwd_ms"]))
        if e:
            L.append("  %-38s %9.2fx   %9.2fx" % ("(a) / bspline_flow", e["eager"]["fwd_ms"] / e["bspline"]["fwd_ms"],
                                                  e["eager"]["bwd_ms"] / e["bspline"]["bwd_ms"]))
            L.append("  bspline_flow against (a) on the first slot (max-abs over max): value %.2e, gradient %.2e" % tuple(e["check"]))
        else:
            L.append("  (a) eager conv_transpose + crop: not measured")
        L.append("  forward: %.1f MB written + read in %.4f ms = %.2f TB/s = %.1f %% of the 8 TB/s HBM peak (a whole-call time: "
                 "launch and allocation included)" % (r["fwd_bytes"] / 1e6, r["bspline"]["fwd_ms"],
                                                      r["fwd_bytes"] / r["bspline"]["fwd_ms"] / 1e9,
                                                      100.0 * r["fwd_bytes"] / (r["bspline"]["fwd_ms"] * 1e-3) / HBM_PEAK))
        duels = [("(b)", r["bspline"], r["linear"])] + ([("(a)", e["bspline"], e["eager"])] if e else [])
        lost = ["%s %s" % (tag, w) for tag, ours, theirs in duels for w, k in (("forward", "fwd_ms"), ("backward", "bwd_ms"))
                if ours[k] >= theirs[k]]
        if lost:
            L.append("  BSPLINE_FLOW DOES NOT BEAT: " + ", ".join(lost))
        L.append("")
    for name in REFINE_VOLS:
        r = res["refine " + name]
        L.append("refine_flow at %s (features='intensity', flow=None, grid_downsize %d, %d iterations), per iteration: 'bspline' "
                 "%.4f ms, 'linear' %.4f ms (%.3fx); rounds %s / %s; similarity first -> last %s."
                 % (name, STRIDE, REFINE_ITERS, r["bspline"]["ms_per_iter"], r["linear"]["ms_per_iter"],
                    r["bspline"]["ms_per_iter"] / r["linear"]["ms_per_iter"], r["bspline"]["rounds"]["ms_per_iter"],
                    r["linear"]["rounds"]["ms_per_iter"], json.dumps(r["similarity"])))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=2, default=None, help="(internal) run one step in this process and print its JSON")
    ap.add_argument("--trace", default=None, choices=sorted(SHAPES), help="only run the ops, for a profiler")
    args = ap.parse_args()
    if args.trace:
        return trace(args.trace)
    fns = {"op": step_op, "eager": step_op, "refine": step_refine}
    if args.step:
        kind, arg = args.step
        print("RESULT " + json.dumps(fns[kind](arg, args.reps, kind)), flush=True)
        return 0
    res = {}
    for kind, arg, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
               "--step", kind, arg]
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:
            print("step %s %s ended with status %d; stopping\n%s" % (kind, arg, out.returncode, out.stderr[-3000:]), flush=True)
            break
        line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1]
        res[kind + " " + arg] = json.loads(line[7:])
        print("%-8s %-16s %s" % (kind, arg, json.dumps(res[kind + " " + arg])), flush=True)
    if not all(k + " " + a in res for k, a, _ in STEPS if k != "eager"):
        return 1
    text = report(res, args.reps)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0 if len(res) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
