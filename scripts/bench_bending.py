"""GPU box: the bending energy (dfmir_amd.ops.bending_energy, csrc/bend.hip) at 1x3x160x192x224 and 16x2x256x256: forward
and forward + backward, beside the same definition composed from eager torch slicing ops on the same GPU and beside the
first-order ops.flow_smoothness(., 'l2'); the achieved bytes/s against the algorithmic traffic (4 B per element read in the
forward, 4 read + 4 written in the backward) as a share of the HBM peak; and a captured 128^3 Registration3DModel step with
regularizer='bending' against 'diffusion', the two alternating in one process.

HIP-event timed per call, medians over `--reps` calls after a warm-up, over a rotating set of fields larger than the
256 MiB last-level cache (every call reads a cold field).  Every step runs in a child process of its own under its own time
limit; a step that fails or runs out of time ends the run (no retries).

    python scripts/bench_bending.py [--reps 20] [--out profiles/bending_timing.txt]
"""
import argparse
import itertools
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
    import math
    import torch
    g = torch.Generator(device=DEV).manual_seed(1)
    n = max(2, -(-COLD_BYTES // (4 * math.prod(shape))))
    return [torch.rand(*shape, device=DEV, generator=g).requires_grad_() for _ in range(n)]


def eager_bending(u):
    """The definition from stock torch slicing ops (the composition the tree could run without the kernels)."""
    nd = u.dim() - 2
    sp = u.shape[2:]

    def at(off):
        return u[(slice(None), slice(None)) + tuple(slice(1 + o, n - 1 + o) for o, n in zip(off, sp))]

    def e(a, s=1):
        return tuple(s if i == a else 0 for i in range(nd))

    def add(p, q):
        return tuple(i + j for i, j in zip(p, q))

    c = at((0,) * nd)
    tot = 0.0
    for a in range(nd):
        tot = tot + (at(e(a)) - 2.0 * c + at(e(a, -1))) ** 2
    for a, b in itertools.combinations(range(nd), 2):
        tot = tot + 2.0 * ((at(add(e(a), e(b))) - at(add(e(a), e(b, -1))) - at(add(e(a, -1), e(b)))
                            + at(add(e(a, -1), e(b, -1)))) / 4.0) ** 2
    return tot.mean()


def step_ops(name, reps):
    import math
    import torch
    from dfmir_amd import ops
    shape = SHAPES[name]
    numel = math.prod(shape)
    fs = fields(shape)
    n = len(fs)
    res = {"fields": n}
    for tag, fn, r in (("bending", ops.bending_energy, reps), ("diffusion_l2", lambda u: ops.flow_smoothness(u, 'l2'), reps),
                       ("eager", eager_bending, max(3, reps // 4))):
        with torch.no_grad():
            fwd = median_ms(lambda i: fn(fs[i % n]), r)
        both = median_ms(lambda i: torch.autograd.grad(fn(fs[i % n]), fs[i % n]), r)
        res[tag] = {"fwd_ms": round(fwd, 4), "fwd_bwd_ms": round(both, 4)}
    # one check beside the timings: the fused value is the eager one
    with torch.no_grad():
        a, b = float(ops.bending_energy(fs[0])), float(eager_bending(fs[0]))
    res["fused_vs_eager_rel"] = abs(a - b) / abs(b)
    f, fb = res["bending"]["fwd_ms"], res["bending"]["fwd_bwd_ms"]
    res["bending"].update(fwd_tbs=round(4 * numel / f / 1e9, 3), fwd_bwd_tbs=round(12 * numel / fb / 1e9, 3),
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
    models = {r: Registration3DModel(shape, device=DEV, capture_step=True, regularizer=r) for r in ("diffusion", "bending")}

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
    out["captured_step_bending_over_diffusion"] = round(out["captured_step_bending_ms"] / out["captured_step_diffusion_ms"], 4)
    return out


STEPS = [("ops", "1x3x160x192x224", 300), ("ops", "16x2x256x256", 240), ("model", "128x128x128", 300)]


def report(res, reps):
    L = ["Bending energy (ops.bending_energy, dfmir_amd/csrc/bend.hip) on one MI355X: output of `python scripts/bench_bending.py "
         "--reps %d`" % reps,
         "(HIP events, medians after a warm-up, fp32, unit spacing; every call reads a field of a rotating set larger than the",
         "256 MiB last-level cache; the eager composition over a quarter of the calls; every step in a child process of its own).",
         "Nothing here is a gate; this is the first measurement.", ""]
    for name in SHAPES:
        r = res[name]
        L.append("%s (%d rotating fields)            forward      forward+backward" % (name, r["fields"]))
        for tag, label in (("bending", "bending_energy (HIP)"), ("diffusion_l2", "flow_smoothness 'l2' (HIP)"),
                           ("eager", "torch-eager composition")):
            L.append("  %-28s %9.4f ms %9.4f ms" % (label, r[tag]["fwd_ms"], r[tag]["fwd_bwd_ms"]))
        L.append("  %-28s %9.1fx   %9.1fx" % ("eager / fused", r["eager"]["fwd_ms"] / r["bending"]["fwd_ms"],
                                               r["eager"]["fwd_bwd_ms"] / r["bending"]["fwd_bwd_ms"]))
        b = r["bending"]
        L.append("  algorithmic traffic (4 B/element forward, 12 B/element forward + backward) over the time: %.3f TB/s = %.1f %% of the "
                 "%.0f TB/s HBM peak forward, %.3f TB/s = %.1f %% forward + backward"
                 % (b["fwd_tbs"], 100 * b["fwd_hbm_frac"], HBM_TBS, b["fwd_bwd_tbs"], 100 * b["fwd_bwd_hbm_frac"]))
        L.append("  fused value against the eager one on the first field: %.2e relative" % r["fused_vs_eager_rel"])
        slower = [w for w, k in (("forward", "fwd_ms"), ("forward + backward", "fwd_bwd_ms")) if r["bending"][k] >= r["eager"][k]]
        if slower:
            L.append("  THE FUSED OP DOES NOT BEAT THE EAGER COMPOSITION HERE: " + ", ".join(slower))
        L.append("")
    m = res["128x128x128"]
    L.append("Registration3DModel 128^3, capture_step=True, default features, the two models stepped alternately in one process: "
             "regularizer='diffusion' %.4f ms per step, regularizer='bending' %.4f ms: %.4fx."
             % (m["captured_step_diffusion_ms"], m["captured_step_bending_ms"], m["captured_step_bending_over_diffusion"]))
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
