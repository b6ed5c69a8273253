"""GPU box: the landmark loss (dfmir_amd.ops.landmark_loss, csrc/landmark.hip) at 1x3x160x192x224 with K = 100 and K = 1000
landmarks: forward and forward + backward (gradient to the flow), beside the composition the tree could run without the
kernels -- F.grid_sample of the flow at the points (align_corners=True) plus torch arithmetic --, the two alternating in one
process; the backward alone (dfmir_landmark_bwd called directly, ten calls back to back between two events, so the device's
time and not the host's launch latency) beside a zero fill of a buffer of dflow's size timed the same way (ops.zero_: the
same grid and 16-byte stores as the backward's own lm_zero_k), i.e. which share of the backward is the zero fill; and a
captured 128^3 Registration3DModel step with landmark_weight=1.0 and K = 100 against the default step, the two alternating in
one process.

HIP-event timed per call, medians over `--reps` calls after a warm-up, over a rotating set of flows larger than the 256 MiB
last-level cache.  Every step runs in a child process of its own under its own time limit; a step that fails or runs out of
time ends the run (no retries).

    python scripts/bench_landmarks.py [--reps 20] [--out profiles/landmark_timing.txt]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DEV = "cuda"
SHAPE = (1, 3, 160, 192, 224)
COLD_BYTES = 640 << 20               # the rotating set of flows holds at least this much
SPACING = (2.0, 1.0, 1.0)


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


def batched_ms(fn, reps, batch=10, warm=3):
    """Per-call time of `batch` calls issued back to back between two events: the queue stays full, so this is the device's
    time per call, not the host's launch latency."""
    return median_ms(lambda i: [fn(i * batch + j) for j in range(batch)], reps, warm) / batch


def make_inputs(K):
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device=DEV).manual_seed(1)
    n = max(2, -(-COLD_BYTES // (4 * math.prod(SHAPE))))
    low = [max(2, s // 8) for s in SHAPE[2:]]
    flows = [F.interpolate(torch.rand(*SHAPE[:2], *low, device=DEV, generator=g) * 6.0 - 3.0, size=SHAPE[2:], mode='trilinear',
                           align_corners=True).contiguous().requires_grad_() for _ in range(n)]
    top = torch.tensor([s - 1 for s in SHAPE[2:]], device=DEV, dtype=torch.float32)
    q = torch.rand(SHAPE[0], K, 3, device=DEV, generator=g) * top
    p = (q + torch.rand(SHAPE[0], K, 3, device=DEV, generator=g) * 6.0 - 3.0).clamp(min=0.0).minimum(top)
    w = 0.5 + torch.rand(SHAPE[0], K, device=DEV, generator=g)
    return flows, q, p, w


def eager_landmark(flow, q, p, w, h):
    """The same loss ('l2') from F.grid_sample and torch arithmetic, validity included."""
    import torch
    import torch.nn.functional as F
    B, nd = flow.shape[:2]
    top = torch.tensor([s - 1 for s in flow.shape[2:]], device=flow.device, dtype=torch.float32)
    valid = (w > 0) & torch.isfinite(q).all(-1) & torch.isfinite(p).all(-1) & (q >= 0).all(-1) & (q <= top).all(-1)
    qs = torch.where(valid[..., None], q, torch.zeros_like(q))
    grid = (2.0 * qs / top - 1.0).flip(-1).reshape((B,) + (1,) * (nd - 1) + (q.shape[1], nd))
    u = F.grid_sample(flow, grid, mode='bilinear', padding_mode='border', align_corners=True)
    m = qs + u.reshape(B, nd, q.shape[1]).transpose(1, 2)
    r = (m - torch.where(valid[..., None], p, torch.zeros_like(p))) * torch.tensor(h, device=flow.device)
    wv = torch.where(valid, w, torch.zeros_like(w))
    return (wv * (r * r).sum(-1)).sum() / wv.sum()


def step_ops(arg, reps):
    import ctypes
    import torch
    from dfmir_amd import lib, ops
    K = int(arg)
    flows, q, p, w = make_inputs(K)
    n = len(flows)
    fused = lambda f: ops.landmark_loss(f, q, p, w, SPACING, 'l2')
    eager = lambda f: eager_landmark(f, q, p, w, SPACING)
    res = {"flows": n}

    def fwd_of(fn):
        with torch.no_grad():
            return median_ms(lambda i: fn(flows[i % n]), max(3, reps))

    def both_of(fn):
        return median_ms(lambda i: torch.autograd.grad(fn(flows[i % n]), flows[i % n]), max(3, reps))
    acc = {k: {"fwd_ms": [], "fwd_bwd_ms": []} for k in ("fused", "eager")}
    for _ in range(3):                                   # the two alternate, three rounds each
        for tag, fn in (("fused", fused), ("eager", eager)):
            acc[tag]["fwd_ms"].append(fwd_of(fn))
            acc[tag]["fwd_bwd_ms"].append(both_of(fn))
    for tag, d in acc.items():
        res[tag] = {k: round(statistics.median(v), 4) for k, v in d.items()}
        res[tag]["rounds"] = {k: [round(x, 4) for x in v] for k, v in d.items()}
    # the backward alone against the zero fill of a buffer of dflow's size
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(2, device=DEV)
    ws = torch.empty(int(lib().dfmir_landmark_ws_floats(3, SHAPE[0], K, *SHAPE[2:])), device=DEV)
    d, per = torch.empty(SHAPE[0], K, device=DEV), torch.empty(SHAPE[0], device=DEV)
    geom = (SHAPE[0], K) + SHAPE[2:] + SPACING + (0,)
    f0 = flows[0].detach()
    assert lib().dfmir_landmark_fwd(3, vp(f0), vp(q), vp(p), vp(w), vp(ws), None, vp(d), vp(per), vp(out), vp(out[1:]), *geom,
                                    st) == 0
    gout = torch.ones(1, device=DEV)
    bufs = [torch.empty_like(f0) for _ in range(n)]

    def bwd(i):
        assert lib().dfmir_landmark_bwd(3, vp(flows[i % n].detach()), vp(q), vp(p), vp(w), vp(gout), vp(out[1:]),
                                        vp(bufs[i % n]), vp(ws), *geom, st) == 0
    res["bwd_ms"] = round(statistics.median([batched_ms(bwd, max(3, reps)) for _ in range(3)]), 4)
    res["zero_ms"] = round(statistics.median([batched_ms(lambda i: ops.zero_(bufs[i % n]), max(3, reps)) for _ in range(3)]), 4)
    # checks beside the timings: the fused value and gradient are the eager ones
    f = flows[0]
    a, b = fused(f), eager(f)
    ga, gb = torch.autograd.grad(a, f)[0], torch.autograd.grad(b, f)[0]
    res["fused_vs_eager_rel"] = abs(float(a) - float(b)) / abs(float(b))
    res["dflow_vs_eager_max_over_max"] = float((ga - gb).abs().max() / gb.abs().max())
    return res


def step_model(_, reps):
    import torch
    from dfmir_amd.registration3d import Registration3DModel
    shape = (128, 128, 128)
    torch.manual_seed(0)
    A = torch.rand(1, 1, *shape, device=DEV)
    B = 0.5 * A + 0.5 * torch.rand(1, 1, *shape, device=DEV)
    b_pts = torch.rand(1, 100, 3, device=DEV) * 127.0
    a_pts = (b_pts + torch.rand(1, 100, 3, device=DEV) * 6.0 - 3.0).clamp(0.0, 127.0)
    models = {"default": Registration3DModel(shape, device=DEV, capture_step=True),
              "landmark": Registration3DModel(shape, device=DEV, capture_step=True, landmark_weight=1.0)}

    def step(m):
        m.set_input({"A": A, "B": B, "A_pts": a_pts, "B_pts": b_pts})
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
    out["losses_landmark"] = models["landmark"].get_current_losses()
    return out


STEPS = [("ops", "100", 300), ("ops", "1000", 300), ("model", "128x128x128", 400)]


def report(res, reps):
    L = ["Landmark loss (ops.landmark_loss, dfmir_amd/csrc/landmark.hip) on one MI355X: output of `python "
         "scripts/bench_landmarks.py --reps %d`" % reps,
         "(HIP events around whole calls, medians after a warm-up, fp32, penalty 'l2', spacing %s, weights given; every call reads a"
         % (SPACING,),
         "flow of a rotating set larger than the 256 MiB last-level cache; fused and eager alternate, three rounds each, the median",
         "of the rounds' medians is shown; every step in a child process of its own).  One call at a time between two events: at",
         "these sizes the fused rows are the host's time to issue two (forward) or five (forward + backward) launches from Python,",
         "not the kernels'; the back-to-back line is closer to the device's own time but still an upper bound (the host issues the",
         "backward's three launches through one ctypes call per backward).  Nothing here is a gate.", ""]
    for K in ("100", "1000"):
        r = res["ops " + K]
        L.append("%s, K = %s (%d rotating flows)              forward      forward+backward" % ("x".join(map(str, SHAPE)), K, r["flows"]))
        for tag, label in (("fused", "landmark_loss (HIP)"), ("eager", "grid_sample + torch arithmetic")):
            L.append("  %-34s %9.4f ms %9.4f ms     rounds fwd %s  fwd+bwd %s"
                     % (label, r[tag]["fwd_ms"], r[tag]["fwd_bwd_ms"], r[tag]["rounds"]["fwd_ms"], r[tag]["rounds"]["fwd_bwd_ms"]))
        L.append("  %-34s %9.2fx   %9.2fx" % ("eager / fused", r["eager"]["fwd_ms"] / r["fused"]["fwd_ms"],
                                              r["eager"]["fwd_bwd_ms"] / r["fused"]["fwd_bwd_ms"]))
        slower = [w for w, k in (("forward", "fwd_ms"), ("forward + backward", "fwd_bwd_ms")) if r["fused"][k] >= r["eager"][k]]
        if slower:
            L.append("  THE FUSED OP DOES NOT BEAT THE EAGER COMPOSITION HERE: " + ", ".join(slower))
        L.append("  device time per call, ten calls back to back: dfmir_landmark_bwd %.4f ms; a zero fill of dflow's %.1f MB alone "
                 "(ops.zero_) %.4f ms = %.0f %% of the backward"
                 % (r["bwd_ms"], 4 * math.prod(SHAPE) / 1e6, r["zero_ms"], 100.0 * r["zero_ms"] / r["bwd_ms"]))
        L.append("  fused against eager on the first flow: value %.2e relative, dflow %.2e (max-abs over max)"
                 % (r["fused_vs_eager_rel"], r["dflow_vs_eager_max_over_max"]))
        L.append("")
    m = res["model 128x128x128"]
    d = m["captured_step_default_ms"]
    L.append("Registration3DModel 128^3, capture_step=True, default features, the two models stepped alternately in one process: "
             "default %.4f ms per step, landmark_weight=1.0 with K = 100 %.4f ms (%.3fx); losses of the last: %s."
             % (d, m["captured_step_landmark_ms"], m["captured_step_landmark_ms"] / d, json.dumps(m["losses_landmark"])))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=2, default=None, help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    fns = {"ops": step_ops, "model": step_model}
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
