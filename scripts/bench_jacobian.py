"""GPU box: the Jacobian-determinant ops (dfmir_amd.ops.jacobian_penalty / jacobian_determinant / jacobian_stats,
csrc/jacdet.hip) at 1x3x160x192x224 and 16x2x256x256: the penalty forward and forward + backward, the map and the
statistics, beside the same definition composed from eager torch slicing ops on the same GPU and beside
ops.bending_energy; the achieved bytes/s against the algorithmic traffic (4 B per element read in the forward, 4 read + 4
written in the backward) as a share of the HBM peak; and a captured 128^3 Registration3DModel step with fold_weight=0.5
against the default model, the two alternating in one process.

HIP-event timed per call, medians over `--reps` calls after a warm-up, over a rotating set of fields larger than the
256 MiB last-level cache (every call reads a cold field).  Every step runs in a child process of its own under its own time
limit; a step that fails or runs out of time ends the run (no retries).

    python scripts/bench_jacobian.py [--reps 20] [--out profiles/jacobian_timing.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_TBS = 8.0
DEV = "cuda"
SHAPES = {"1x3x160x192x224": (1, 3, 160, 192, 224), "16x2x256x256": (16, 2, 256, 256)}
COLD_BYTES = 640 << 20               # the rotating set of a shape holds at least this much
EPS, POWER = 0.5, 2
# hipcc -Rpass-analysis=kernel-resource-usage on jacdet.hip (gfx950): what the kernels were built with
RESOURCES = """Compile-time budget (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no kernel spills to scratch):
  jac_fwd_k<3-D>  LDS 25 920 B (three open planes of three channels at 10 x 72 floats) + the reduction slots; VGPRs vector /
                  scalar staging: penalty 80 / 74, map 60 / 56, statistics 88 / 82
  jac_fwd_k<2-D>  LDS 5 760 B; VGPRs 18 to 20 (penalty, map), 45 / 46 (statistics)
  jac_bwd_k<3-D>  LDS 46 944 B = 31 104 (three open planes of three channels at 12 x 72 floats) + 15 840 (the y and x columns of
                  W of ONE plane over tile + 1, 2 x 3 x 10 x 66 floats); the z column of W stays in registers (three planes x two
                  voxels x three channels), so u needs three open planes, not five, and no W window in LDS: 3 workgroups per CU;
                  VGPRs 109 (vector) / 115 (scalar)
  jac_bwd_k<2-D>  LDS 17 472 B; VGPRs 22"""


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


def fields(shape):
    """Seeded uniform noise of up to 3 voxels: part of the voxels fold, so the hinge is active (the report says how many)."""
    import math
    import torch
    g = torch.Generator(device=DEV).manual_seed(1)
    n = max(2, -(-COLD_BYTES // (4 * math.prod(shape))))
    return [(3.0 * torch.rand(*shape, device=DEV, generator=g)).requires_grad_() for _ in range(n)]


def eager_det(u):
    """det J from stock torch slicing ops (the composition the tree could run without the kernels), on Omega_1."""
    nd, sp = u.dim() - 2, u.shape[2:]

    def at(a, b, s):
        return u[(slice(None), a) + tuple(slice(1 + (s if i == b else 0), n - 1 + (s if i == b else 0)) for i, n in enumerate(sp))]

    J = [[(at(a, b, 1) - at(a, b, -1)) / 2.0 + (1.0 if a == b else 0.0) for b in range(nd)] for a in range(nd)]
    if nd == 2:
        return J[0][0] * J[1][1] - J[0][1] * J[1][0]
    return (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) + J[0][1] * (J[1][2] * J[2][0] - J[1][0] * J[2][2])
            + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))


def eager_penalty(u):
    import torch
    return torch.clamp(EPS - eager_det(u), min=0.0).square().mean()


def eager_stats(u):
    import torch
    d = eager_det(u).reshape(u.shape[0], -1)
    l = torch.log(torch.clamp(d + 3.0, min=1e-9))
    return torch.stack([(d <= 0).double().sum(1), d.min(1).values.double(), d.max(1).values.double(), d.double().mean(1),
                        l.double().mean(1), l.double().std(1, unbiased=False)], 1)


def step_ops(name, reps):
    import math
    import torch
    from dfmir_amd import ops
    shape = SHAPES[name]
    numel = math.prod(shape)
    fs = fields(shape)
    n = len(fs)
    res = {"fields": n}
    pen = lambda u: ops.jacobian_penalty(u, EPS, POWER)
    for tag, fn, r in (("penalty", pen, reps), ("bending", ops.bending_energy, reps), ("eager", eager_penalty, max(3, reps // 4))):
        with torch.no_grad():
            fwd = median_ms(lambda i: fn(fs[i % n]), r)
        both = median_ms(lambda i: torch.autograd.grad(fn(fs[i % n]), fs[i % n]), r)
        res[tag] = {"fwd_ms": round(fwd, 4), "fwd_bwd_ms": round(both, 4)}
    with torch.no_grad():
        res["map_ms"] = round(median_ms(lambda i: ops.jacobian_determinant(fs[i % n]), reps), 4)
        res["stats_ms"] = round(median_ms(lambda i: ops.jacobian_stats(fs[i % n], 1, 3.0), reps), 4)
        res["eager_map_ms"] = round(median_ms(lambda i: eager_det(fs[i % n]), max(3, reps // 4)), 4)
        res["eager_stats_ms"] = round(median_ms(lambda i: eager_stats(fs[i % n]), max(3, reps // 4)), 4)
        # two checks beside the timings: the fused values are the eager ones
        a, b = float(pen(fs[0])), float(eager_penalty(fs[0]))
        res["fused_vs_eager_rel"] = abs(a - b) / abs(b)
        res["folded_fraction"] = float(ops.jacobian_stats(fs[0])[0, 0]) / (numel / shape[0] / shape[1])
        res["stats_vs_eager_abs"] = float((ops.jacobian_stats(fs[0], 1, 3.0) - eager_stats(fs[0])).abs()[:, 1:].max())
    f, fb = res["penalty"]["fwd_ms"], res["penalty"]["fwd_bwd_ms"]
    res["penalty"].update(fwd_tbs=round(4 * numel / f / 1e9, 3), fwd_bwd_tbs=round(12 * numel / fb / 1e9, 3),
                          fwd_hbm_frac=round(4 * numel / f / 1e9 / HBM_TBS, 4),
                          fwd_bwd_hbm_frac=round(12 * numel / fb / 1e9 / HBM_TBS, 4))
    return res


def step_model(_, reps):
    import torch
    from dfmir_amd.registration3d import Registration3DModel
    shape = (128, 128, 128)
    torch.manual_seed(0)
    A = torch.rand(1, 1, *shape, device=DEV)
    B = 0.5 * A + 0.5 * torch.rand(1, 1, *shape, device=DEV)
    models = {"plain": Registration3DModel(shape, device=DEV, capture_step=True),
              "fold": Registration3DModel(shape, device=DEV, capture_step=True, fold_weight=0.5, fold_eps=EPS)}

    def step(m):
        m.set_input({"A": A, "B": B})
        m.optimize_parameters()
    for m in models.values():
        for _ in range(5):
            step(m)
        assert m._graph['graph'] is not None
    torch.cuda.synchronize()
    ts = {r: [] for r in models}
    for _ in range(reps):
        for r, m in models.items():                      # alternating
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            step(m)
            e.record()
            e.synchronize()
            ts[r].append(s.elapsed_time(e))
    out = {"captured_step_%s_ms" % r: round(statistics.median(v), 4) for r, v in ts.items()}
    out["captured_step_fold_over_plain"] = round(out["captured_step_fold_ms"] / out["captured_step_plain_ms"], 4)
    return out


STEPS = [("ops", "1x3x160x192x224", 300), ("ops", "16x2x256x256", 240), ("model", "128x128x128", 300)]


def report(res, reps):
    L = ["Jacobian determinant (ops.jacobian_penalty / jacobian_determinant / jacobian_stats, dfmir_amd/csrc/jacdet.hip) on one MI355X:",
         "output of `python scripts/bench_jacobian.py --reps %d`" % reps,
         "(HIP events, medians after a warm-up, fp32, penalty with eps = %.1f and power = %d, border 1; every call reads a field of a"
         % (EPS, POWER),
         "rotating set larger than the 256 MiB last-level cache; the eager composition over a quarter of the calls; every step in a",
         "child process of its own).  Nothing here is a gate; this is the first measurement.  The times are measured from the host",
         "around whole calls (allocation of the result, the autograd node and the launches included).", ""]
    for name in SHAPES:
        r = res[name]
        L.append("%s (%d rotating fields, %.1f %% of the voxels folded)   forward      forward+backward"
                 % (name, r["fields"], 100 * r["folded_fraction"]))
        for tag, label in (("penalty", "jacobian_penalty (HIP)"), ("bending", "bending_energy (HIP)"),
                           ("eager", "torch-eager composition")):
            L.append("  %-28s %9.4f ms %9.4f ms" % (label, r[tag]["fwd_ms"], r[tag]["fwd_bwd_ms"]))
        L.append("  %-28s %9.1fx   %9.1fx" % ("eager / fused", r["eager"]["fwd_ms"] / r["penalty"]["fwd_ms"],
                                               r["eager"]["fwd_bwd_ms"] / r["penalty"]["fwd_bwd_ms"]))
        L.append("  jacobian_determinant %.4f ms (eager %.4f ms), jacobian_stats %.4f ms (eager %.4f ms)"
                 % (r["map_ms"], r["eager_map_ms"], r["stats_ms"], r["eager_stats_ms"]))
        b = r["penalty"]
        L.append("  algorithmic traffic (4 B/element forward, 12 B/element forward + backward) over the time: %.3f TB/s = %.1f %% of the "
                 "%.0f TB/s HBM peak forward, %.3f TB/s = %.1f %% forward + backward"
                 % (b["fwd_tbs"], 100 * b["fwd_hbm_frac"], HBM_TBS, b["fwd_bwd_tbs"], 100 * b["fwd_bwd_hbm_frac"]))
        L.append("  fused penalty against the eager one on the first field: %.2e relative; statistics (min, max, means, std): %.2e absolute"
                 % (r["fused_vs_eager_rel"], r["stats_vs_eager_abs"]))
        slower = [w for w, k in (("forward", "fwd_ms"), ("forward + backward", "fwd_bwd_ms")) if r["penalty"][k] >= r["eager"][k]]
        if slower:
            L.append("  THE FUSED OP DOES NOT BEAT THE EAGER COMPOSITION HERE: " + ", ".join(slower))
        L.append("")
    m = res["128x128x128"]
    L.append("Registration3DModel 128^3, capture_step=True, default features, the two models stepped alternately in one process: "
             "default %.4f ms per step, fold_weight=0.5 %.4f ms: %.4fx."
             % (m["captured_step_plain_ms"], m["captured_step_fold_ms"], m["captured_step_fold_over_plain"]))
    L += ["", RESOURCES]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=2, default=None, help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        kind, arg = args.step
        print("RESULT " + json.dumps({"ops": step_ops, "model": step_model}[kind](arg, args.reps)), flush=True)
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
        res[arg] = json.loads(line[7:])
        print("%-6s %-16s %s" % (kind, arg, json.dumps(res[arg])), flush=True)
    text = report(res, args.reps)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
