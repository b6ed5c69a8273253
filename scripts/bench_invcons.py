"""GPU box: the inverse-consistency loss (dfmir_amd.ops.inverse_consistency, csrc/invcons.hip) at 1x3x160x192x224 and
16x2x256x256: forward and forward + backward (gradients to both fields), beside the composition the tree could run without
the kernels -- ops.warp, add, ops.mul, ops.mean -- and beside the same op with DFMIR_INVCONS_FIXED64 set (dv through the 64-bit
fixed-point scatter on every shape), alternating in one process; the kernel times of a rocprofv3 --kernel-trace --stats run
of its own against the algorithmic traffic (forward 2 * 4 * nd * S * B bytes: u read, v gathered; backward twice that -- u, v
read, du, k r written -- plus the dv pass) as a share of the HBM peak; and a captured 128^3 Registration3DModel step with
symmetric=True, with and without inverse_consistency=0.1, against the default step, the three alternating in one process.

HIP-event timed per call, medians over `--reps` calls after a warm-up, over a rotating set of field pairs larger than the
256 MiB last-level cache (every call reads cold fields).  The fields are a registration-like near-inverse pair: u a smooth
displacement of up to 3 voxels (noise at 1/8 resolution, linearly up-sampled), v = -u plus 10 % noise.  Every step runs in a
child process of its own under its own time limit; a step that fails or runs out of time ends the run (no retries).

    python scripts/bench_invcons.py [--reps 20] [--out profiles/invcons_timing.txt]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_TBS = 8.0
DEV = "cuda"
SHAPES = {"1x3x160x192x224": (1, 3, 160, 192, 224), "16x2x256x256": (16, 2, 256, 256)}
COLD_BYTES = 640 << 20               # the rotating set of a shape holds at least this much
KERNEL_CALLS = 10                    # forward + backward calls of the traced run


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


def pairs(shape, cold_bytes=COLD_BYTES):
    import math
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device=DEV).manual_seed(1)
    n = max(2, -(-cold_bytes // (8 * math.prod(shape))))
    out = []
    for _ in range(n):
        low = [max(2, s // 8) for s in shape[2:]]
        u = F.interpolate(torch.rand(*shape[:2], *low, device=DEV, generator=g) * 6.0 - 3.0, size=shape[2:],
                          mode='trilinear' if len(shape) == 5 else 'bilinear', align_corners=True).contiguous()
        v = -u + 0.3 * (2.0 * torch.rand(*shape, device=DEV, generator=g) - 1.0)
        out.append((u.requires_grad_(), v.requires_grad_()))
    return out


def eager_ic(u, v):
    """The composition from the ops the tree had before the fused kernels: four launches forward, four back."""
    from dfmir_amd import ops
    r = u + ops.warp(v, u)
    return ops.mean(ops.mul(r, r))


def step_ops(name, reps):
    import torch
    from dfmir_amd import _lib, ops
    shape = SHAPES[name]
    ps = pairs(shape)
    n = len(ps)
    res = {"pairs": n}

    def fwd_of(fn):
        with torch.no_grad():
            return median_ms(lambda i: fn(*ps[i % n]), max(3, reps))

    def both_of(fn):
        return median_ms(lambda i: torch.autograd.grad(fn(*ps[i % n]), ps[i % n]), max(3, reps))
    acc = {k: {"fwd_ms": [], "fwd_bwd_ms": []} for k in ("fused", "fused_fixed64", "eager")}
    for _ in range(3):                                   # the three alternate, three rounds each
        for tag in acc:
            _lib.set_option("DFMIR_INVCONS_FIXED64", "1" if tag == "fused_fixed64" else None)
            fn = eager_ic if tag == "eager" else ops.inverse_consistency
            acc[tag]["fwd_ms"].append(fwd_of(fn))
            acc[tag]["fwd_bwd_ms"].append(both_of(fn))
    _lib.set_option("DFMIR_INVCONS_FIXED64", None)
    for tag, d in acc.items():
        res[tag] = {k: round(statistics.median(v), 4) for k, v in d.items()}
        res[tag]["rounds"] = {k: [round(x, 4) for x in v] for k, v in d.items()}
    # checks beside the timings: the fused value and gradients are the eager ones
    u, v = ps[0]
    a, b = ops.inverse_consistency(u, v), eager_ic(u, v)
    ga, gb = torch.autograd.grad(a, (u, v)), torch.autograd.grad(b, (u, v))
    res["fused_vs_eager_rel"] = abs(float(a) - float(b)) / abs(float(b))
    res["du_vs_eager_max_over_max"] = float((ga[0] - gb[0]).abs().max() / gb[0].abs().max())
    res["dv_vs_eager_max_over_max"] = float((ga[1] - gb[1]).abs().max() / gb[1].abs().max())
    return res


def step_trace(name, _):
    """KERNEL_CALLS forward + backward calls on rotating cold pairs: the process rocprofv3 traces (the dv path comes from the
    environment variable DFMIR_INVCONS_FIXED64)."""
    import torch
    from dfmir_amd import ops
    ps = pairs(SHAPES[name])
    for i in range(KERNEL_CALLS):
        u, v = ps[i % len(ps)]
        torch.autograd.grad(ops.inverse_consistency(u, v), (u, v))
    torch.cuda.synchronize()
    return {}


def step_kernels(name, reps):
    """Average duration of every kernel of invcons.hip and of the owner-gather adjoint, from rocprofv3's kernel stats: one
    traced run per dv path."""
    res = {}
    for path, opt in (("owner-gather dv", None), ("fixed-point dv", "1")):
        env = dict(os.environ)
        env.pop("DFMIR_INVCONS_FIXED64", None)
        if opt:
            env["DFMIR_INVCONS_FIXED64"] = opt
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.abspath(__file__), "--step", "trace", name]
            out = subprocess.run(cmd, capture_output=True, text=True, env=env)
            if out.returncode != 0:
                raise RuntimeError("rocprofv3 run failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                raise RuntimeError("no kernel_stats.csv under %s" % d)
            res[path] = {}
            with open(files[0]) as fh:
                for row in csv.DictReader(fh):
                    nm = row["Name"]
                    if any(k in nm for k in ("ic_fwd_k", "ic_bwd_k", "ic_fin_k", "ic_zero_k", "ic_cvt_k", "warp_win_bwd_own_k",
                                             "warp_win_gather_k", "warp_win_slow_k")):
                        short = nm.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
                        res[path][short] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                                            "min_us": round(float(row["MinNs"]) / 1e3, 2)}
    return res


def step_model(_, reps):
    import torch
    from dfmir_amd.registration3d import Registration3DModel
    shape = (128, 128, 128)
    torch.manual_seed(0)
    A = torch.rand(1, 1, *shape, device=DEV)
    B = 0.5 * A + 0.5 * torch.rand(1, 1, *shape, device=DEV)
    models = {"default": Registration3DModel(shape, device=DEV, capture_step=True),
              "symmetric": Registration3DModel(shape, device=DEV, capture_step=True, symmetric=True),
              "symmetric_ic": Registration3DModel(shape, device=DEV, capture_step=True, symmetric=True, inverse_consistency=0.1)}

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
    out["losses_symmetric_ic"] = models["symmetric_ic"].get_current_losses()
    return out


STEPS = [("ops", "1x3x160x192x224", 400), ("ops", "16x2x256x256", 300), ("kernels", "1x3x160x192x224", 300),
         ("kernels", "16x2x256x256", 300), ("model", "128x128x128", 400)]


def _traffic(shape):
    """(forward bytes, backward bytes without the dv pass) of the algorithmic traffic."""
    import math
    f = 2 * 4 * math.prod(shape)
    return f, 2 * f


def report(res, reps):
    L = ["Inverse-consistency loss (ops.inverse_consistency, dfmir_amd/csrc/invcons.hip) on one MI355X: output of `python "
         "scripts/bench_invcons.py --reps %d`" % reps,
         "(HIP events around whole calls, medians after a warm-up, fp32; every call reads a pair of a rotating set larger than the",
         "256 MiB last-level cache; fused, fused with DFMIR_INVCONS_FIXED64 and the eager composition alternate, three rounds each,",
         "the median of the rounds' medians is shown; every step in a child process of its own).  Nothing here is a gate.", ""]
    for name in SHAPES:
        r = res["ops " + name]
        L.append("%s (%d rotating pairs)                       forward      forward+backward" % (name, r["pairs"]))
        for tag, label in (("fused", "inverse_consistency (HIP)"), ("fused_fixed64", "  with DFMIR_INVCONS_FIXED64"),
                           ("eager", "ops.warp, +, ops.mul, ops.mean")):
            L.append("  %-34s %9.4f ms %9.4f ms     rounds fwd %s  fwd+bwd %s"
                     % (label, r[tag]["fwd_ms"], r[tag]["fwd_bwd_ms"], r[tag]["rounds"]["fwd_ms"], r[tag]["rounds"]["fwd_bwd_ms"]))
        L.append("  %-34s %9.2fx   %9.2fx" % ("eager / fused", r["eager"]["fwd_ms"] / r["fused"]["fwd_ms"],
                                              r["eager"]["fwd_bwd_ms"] / r["fused"]["fwd_bwd_ms"]))
        L.append("  fused against eager on the first pair: value %.2e relative, du %.2e, dv %.2e (max-abs over max)"
                 % (r["fused_vs_eager_rel"], r["du_vs_eager_max_over_max"], r["dv_vs_eager_max_over_max"]))
        slower = [w for w, k in (("forward", "fwd_ms"), ("forward + backward", "fwd_bwd_ms")) if r["fused"][k] >= r["eager"][k]]
        if slower:
            L.append("  THE FUSED OP DOES NOT BEAT THE EAGER COMPOSITION HERE: " + ", ".join(slower))
        fb, bb = _traffic(SHAPES[name])
        L.append("  kernels (rocprofv3 --kernel-trace --stats, one run of its own per dv path: %d forward + backward calls on cold "
                 "pairs; average / minimum):" % KERNEL_CALLS)
        for path, k in res["kernels " + name].items():
            L.append("   %s" % path)
            for nm in sorted(k):
                extra = ""
                if "ic_fwd_k" in nm or "ic_bwd_k" in nm:
                    nb = fb if "ic_fwd_k" in nm else bb
                    extra = "   %.1f MB algorithmic%s: %.2f TB/s = %.1f %% of the %.0f TB/s HBM peak" % (
                        nb / 1e6, "" if "ic_fwd_k" in nm else " (without the dv pass)", nb / k[nm]["avg_us"] / 1e6,
                        100 * nb / k[nm]["avg_us"] / 1e6 / HBM_TBS, HBM_TBS)
                L.append("    %-34s x%-4d %9.2f us %9.2f us%s" % (nm, k[nm]["calls"], k[nm]["avg_us"], k[nm]["min_us"], extra))
        L.append("")
    m = res["model 128x128x128"]
    d = m["captured_step_default_ms"]
    L.append("Registration3DModel 128^3, capture_step=True, default features, the three models stepped alternately in one process: "
             "default %.4f ms per step, symmetric=True %.4f ms (%.3fx), symmetric=True with inverse_consistency=0.1 %.4f ms (%.3fx); "
             "losses of the last: %s."
             % (d, m["captured_step_symmetric_ms"], m["captured_step_symmetric_ms"] / d, m["captured_step_symmetric_ic_ms"],
                m["captured_step_symmetric_ic_ms"] / d, json.dumps(m["losses_symmetric_ic"])))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=2, default=None, help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    fns = {"ops": step_ops, "trace": step_trace, "kernels": step_kernels, "model": step_model}
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
