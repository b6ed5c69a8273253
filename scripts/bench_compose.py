"""GPU box: flow composition and fixed-point inversion (dfmir_amd.ops.compose_flows / invert_flow, csrc/compose.hip) at
1x3x160x192x224 and 16x2x256x256, beside what the tree could run without the kernels:
  compose_flows   forward and forward + backward (gradients to both fields) against u + ops.warp(v, u) and its autograd;
  invert_flow     iters=20, plain, with history=True and with tol=1e-3, against the eager loop w = ops.scale(ops.warp(u, w),
                  -1.0) x 20 (a warp and a negation per iteration: the field written and re-read twice per iteration);
  refine_flow     at 128^3 with a starting flow, update='compose' against update='add', per iteration;
and one unchanged `python bench.py --gpus 1 --steps 20 --warmup 5` line: the default step runs none of the new code.

HIP-event timed per call, medians over `--reps` calls after a warm-up, over a rotating set of fields larger than the 256 MiB
last-level cache (every call reads cold fields); the sides alternate in one process, three rounds each, and the median of the
rounds' medians is shown.  The fields are registration-like: u a smooth displacement of up to 3 voxels (noise at 1/8
resolution, linearly up-sampled), v = -u plus 10 % noise.  Every step runs in a child process of its own under its own time
limit; a step that fails or runs out of time ends the run (no retries).  Nothing here is a gate.

    python scripts/bench_compose.py [--reps 20] [--out profiles/compose_timing.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from scripts.bench_invcons import COLD_BYTES, DEV, SHAPES, median_ms, pairs  # noqa: E402

ITERS = 20
TOL = 1e-3
REFINE_VOL = (128, 128, 128)
REFINE_ITERS = 10


def eager_compose(u, v):
    from dfmir_amd import ops
    return u + ops.warp(v, u)


def eager_invert(u, iters=ITERS):
    from dfmir_amd import ops
    w = ops.zeros_like(u)
    for _ in range(iters):
        w = ops.scale(ops.warp(u, w), -1.0)
    return w


def _rounds(sides, measure, rounds=3):
    """{tag: {key: median of the rounds' medians, 'rounds': ...}} with the sides alternating"""
    acc = {tag: {} for tag in sides}
    for _ in range(rounds):
        for tag, fn in sides.items():
            for key, ms in measure(fn).items():
                acc[tag].setdefault(key, []).append(ms)
    return {tag: dict({k: round(statistics.median(v), 4) for k, v in d.items()},
                      rounds={k: [round(x, 4) for x in v] for k, v in d.items()}) for tag, d in acc.items()}


def step_compose(name, reps):
    import torch
    from dfmir_amd import ops
    ps = pairs(SHAPES[name])
    n = len(ps)
    gs = [torch.rand_like(u) for u, _ in ps]

    def measure(fn):
        with torch.no_grad():
            f = median_ms(lambda i: fn(*ps[i % n]), max(3, reps))
        b = median_ms(lambda i: torch.autograd.grad(fn(*ps[i % n]), ps[i % n], gs[i % n]), max(3, reps))
        return {"fwd_ms": f, "fwd_bwd_ms": b}
    res = _rounds({"fused": ops.compose_flows, "eager": eager_compose}, measure)
    res["pairs"] = n
    u, v = ps[0]
    a, b = ops.compose_flows(u, v), eager_compose(u, v)
    ga, gb = torch.autograd.grad(a, (u, v), gs[0]), torch.autograd.grad(b, (u, v), gs[0])
    res["check"] = [float((x - y).abs().max() / y.abs().max()) for x, y in ((a, b), (ga[0], gb[0]), (ga[1], gb[1]))]
    return res


def step_invert(name, reps):
    import torch
    from dfmir_amd import ops
    us = [u.detach() for u, _ in pairs(SHAPES[name], COLD_BYTES // 2)]
    n = len(us)
    sides = {"fused": lambda u: ops.invert_flow(u, iters=ITERS),
             "fused_history": lambda u: ops.invert_flow(u, iters=ITERS, history=True),
             "fused_tol": lambda u: ops.invert_flow(u, iters=ITERS, tol=TOL),
             "eager": eager_invert}
    with torch.no_grad():
        res = _rounds(sides, lambda fn: {"ms": median_ms(lambda i: fn(us[i % n]), max(3, reps))})
        res["fields"] = n
        w, hist = ops.invert_flow(us[0], iters=ITERS, history=True)
        e = eager_invert(us[0])
        res["check"] = float((w - e).abs().max() / e.abs().max())
        res["rms"] = [float(x) for x in hist[:, :, 0].max(1).values.cpu()]
        wt, st = ops.invert_flow(us[0], iters=ITERS, tol=TOL)
        res["tol_stopped_share"] = float((ops.compose_flows(wt, us[0]).abs().amax(1) <= TOL).float().mean())
    return res


def step_refine(_, reps):
    import torch
    import torch.nn.functional as F
    from dfmir_amd import infer
    torch.manual_seed(0)
    vol = REFINE_VOL
    A = torch.rand(1, 1, *vol, device=DEV)
    B = 0.5 * A + 0.5 * torch.rand(1, 1, *vol, device=DEV)
    flow0 = F.interpolate(torch.rand(1, 3, 16, 16, 16, device=DEV) * 4.0 - 2.0, size=vol, mode='trilinear',
                          align_corners=True).contiguous()
    kw = dict(features='intensity', lam=0.05, lr=0.1, iters=REFINE_ITERS)
    sides = {u: (lambda u=u: infer.refine_flow(A, B, flow0, update=u, **kw)) for u in ("compose", "add")}
    res = _rounds(sides, lambda fn: {"ms_per_iter": median_ms(lambda i: fn(), max(3, reps // 4), warm=1) / REFINE_ITERS})
    res["final_similarity"] = {u: float(fn()["history"][-1, 0]) for u, fn in sides.items()}
    return res


def step_bench(_, reps):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                         capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("bench.py ended with status %d: %s" % (out.returncode, out.stderr[-2000:]))
    return {"line": [l for l in out.stdout.splitlines() if l.startswith("{")][-1]}


STEPS = [("compose", "1x3x160x192x224", 400), ("compose", "16x2x256x256", 300), ("invert", "1x3x160x192x224", 400),
         ("invert", "16x2x256x256", 300), ("refine", "128x128x128", 400), ("bench", "default", 600)]


def report(res, reps):
    L = ["Flow composition and fixed-point inversion (ops.compose_flows / ops.invert_flow, dfmir_amd/csrc/compose.hip) on one "
         "MI355X: output of `python scripts/bench_compose.py --reps %d`" % reps,
         "(HIP events around whole calls, medians after a warm-up, fp32; every call reads fields of a rotating set larger than the",
         "256 MiB last-level cache; the sides alternate, three rounds each, the median of the rounds' medians is shown; every step",
         "in a child process of its own).  Nothing here is a gate.", ""]
    for name in SHAPES:
        r = res["compose " + name]
        L.append("%s (%d rotating pairs)                       forward      forward+backward" % (name, r["pairs"]))
        for tag, label in (("fused", "compose_flows (HIP)"), ("eager", "u + ops.warp(v, u)")):
            L.append("  %-34s %9.4f ms %9.4f ms     rounds fwd %s  fwd+bwd %s"
                     % (label, r[tag]["fwd_ms"], r[tag]["fwd_bwd_ms"], r[tag]["rounds"]["fwd_ms"], r[tag]["rounds"]["fwd_bwd_ms"]))
        L.append("  %-34s %9.2fx   %9.2fx" % ("eager / fused", r["eager"]["fwd_ms"] / r["fused"]["fwd_ms"],
                                              r["eager"]["fwd_bwd_ms"] / r["fused"]["fwd_bwd_ms"]))
        L.append("  fused against eager on the first pair (max-abs over max): value %.2e, du %.2e, dv %.2e" % tuple(r["check"]))
        slower = [w for w, k in (("forward", "fwd_ms"), ("forward + backward", "fwd_bwd_ms")) if r["fused"][k] >= r["eager"][k]]
        if slower:
            L.append("  THE FUSED OP DOES NOT BEAT THE EAGER COMPOSITION HERE: " + ", ".join(slower))
        r = res["invert " + name]
        L.append("  invert_flow, %d iterations (%d rotating fields)" % (ITERS, r["fields"]))
        for tag, label in (("fused", "invert_flow (HIP, one launch)"), ("fused_history", "  with history=True"),
                           ("fused_tol", "  with tol=%g" % TOL), ("eager", "ops.warp, ops.scale x %d" % ITERS)):
            L.append("  %-34s %9.4f ms                  rounds %s" % (label, r[tag]["ms"], r[tag]["rounds"]["ms"]))
        L.append("  %-34s %9.2fx" % ("eager / fused", r["eager"]["ms"] / r["fused"]["ms"]))
        L.append("  fused against the eager loop on the first field: %.2e (max-abs over max); rms_k of it: %s; with tol the share of "
                 "voxels that end at or below it: %.3f" % (r["check"], " ".join("%.1e" % x for x in r["rms"]), r["tol_stopped_share"]))
        if r["fused"]["ms"] >= r["eager"]["ms"]:
            L.append("  THE SINGLE-LAUNCH INVERSION DOES NOT BEAT THE EAGER LOOP HERE")
        L.append("")
    r = res["refine 128x128x128"]
    L.append("refine_flow at 128^3 (features='intensity', a starting flow of up to 2 voxels, %d iterations), per iteration: "
             "update='compose' %.4f ms, update='add' %.4f ms (%.3fx); rounds %s / %s; final similarity %s."
             % (REFINE_ITERS, r["compose"]["ms_per_iter"], r["add"]["ms_per_iter"],
                r["compose"]["ms_per_iter"] / r["add"]["ms_per_iter"], r["compose"]["rounds"]["ms_per_iter"],
                r["add"]["rounds"]["ms_per_iter"], json.dumps(r["final_similarity"])))
    L.append("")
    L.append("python bench.py --gpus 1 --steps 20 --warmup 5 (unchanged; the default step runs none of the new code):")
    L.append(res["bench default"]["line"])
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=2, default=None, help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    fns = {"compose": step_compose, "invert": step_invert, "refine": step_refine, "bench": step_bench}
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
        print("%-8s %-16s %s" % (kind, arg, json.dumps(res[kind + " " + arg])), flush=True)
    text = report(res, args.reps)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
