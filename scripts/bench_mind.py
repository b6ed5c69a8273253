"""GPU box: the MIND-SSC loss (dfmir_amd.ops.mind_loss, csrc/mind.hip) at 160x192x224 and 128^3: forward and forward +
backward, beside the box NCC loss of the same size; the same definition composed from eager torch ops on the same GPU
(replicate padding, slicing, avg_pool3d, min, clamp, exp); and a captured 128^3 Registration3DModel step with
similarity='mind' against 'ncc'.  HIP-event timed per call, medians over `--reps` calls after a warm-up, over a rotating set
of image pairs.

Every step runs in a child process of its own under its own time limit; a step that fails or runs out of time ends the
run (no retries).

    python scripts/bench_mind.py [--reps 20] [--out profiles/mind_bench.json]
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
SHAPES = {"160x192x224": (160, 192, 224), "128x128x128": (128, 128, 128)}
# bytes per voxel (3-D, C = 12 channels of fp32; halo re-reads not counted).  Algorithmic minimum: read both images in the
# forward, read them again and write both gradients in the backward.  This implementation stores m (C floats per voxel and
# image) and runs the backward through two C-channel scratch volumes per image.
MIN_FWD, MIN_FWD_BWD = 8, 24
OUR_FWD = 2 * (4 + 48) + 2 * 48                            # pass A per image: read I, write m; loss pass: read both m
OUR_BWD = 2 * ((2 * 48 + 48) + (48 + 48) + (48 + 4 + 4))   # per image: dL/dD, its box adjoint, the shift adjoint


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


def pairs(shape, n):
    import torch
    g = torch.Generator(device=DEV).manual_seed(1)
    out = []
    for _ in range(n):
        a = torch.rand(1, 1, *shape, device=DEV, generator=g)
        b = 0.5 * a + 0.5 * torch.rand(1, 1, *shape, device=DEV, generator=g)
        out.append((a.requires_grad_(), b.requires_grad_()))
    return out


def eager_mind(I, r=2, d=2):
    """The definition from stock torch ops (the composition the tree could run without the kernels)."""
    import torch
    import torch.nn.functional as F
    Ip = F.pad(I, (d,) * 6, mode='replicate')
    sp = I.shape[2:]

    def shifted(n):
        sl = [slice(None), slice(None)] + [slice(d, d + e) for e in sp]
        o = d + (d if n & 1 else -d)
        sl[2 + n // 2] = slice(o, o + sp[n // 2])
        return Ip[tuple(sl)]

    ch = [(p, q) for p in range(6) for q in range(p + 1, 6) if p // 2 != q // 2]
    Dm = torch.cat([F.avg_pool3d(F.pad((shifted(p) - shifted(q)) ** 2, (r,) * 6, mode='replicate'), 2 * r + 1, stride=1)
                    for p, q in ch], 1)
    m = Dm - Dm.min(1, keepdim=True).values
    V = m.mean(1, keepdim=True)
    mu = V.mean().detach()
    return torch.exp(-m / V.clamp(min=0.001 * mu, max=1000.0 * mu))


def step_kernels(name, reps):
    import torch
    from dfmir_amd import ops
    shape = SHAPES[name]
    V = shape[0] * shape[1] * shape[2]
    ps = pairs(shape, 4)
    n = len(ps)
    res = {}
    for tag, fn in (("mind", lambda a, b: ops.mind_loss(a, b)), ("ncc_box", lambda a, b: ops.ncc_loss(a, b, 9))):
        with torch.no_grad():
            fwd = median_ms(lambda i: fn(*ps[i % n]), reps)
        both = median_ms(lambda i: torch.autograd.grad(fn(*ps[i % n]), ps[i % n][:2 if tag == "mind" else 1]), reps)
        res[tag] = {"fwd_ms": round(fwd, 4), "fwd_bwd_ms": round(both, 4)}
    f, fb = res["mind"]["fwd_ms"], res["mind"]["fwd_bwd_ms"]
    res["mind"].update(
        fwd_bytes_per_voxel=OUR_FWD, fwd_bwd_bytes_per_voxel=OUR_FWD + OUR_BWD, min_fwd_bytes_per_voxel=MIN_FWD,
        min_fwd_bwd_bytes_per_voxel=MIN_FWD_BWD,
        fwd_hbm_frac=round(V * OUR_FWD / f / 1e9 / HBM_TBS, 4), fwd_bwd_hbm_frac=round(V * (OUR_FWD + OUR_BWD) / fb / 1e9 / HBM_TBS, 4),
        fwd_hbm_frac_of_min=round(V * MIN_FWD / f / 1e9 / HBM_TBS, 5), fwd_bwd_hbm_frac_of_min=round(V * MIN_FWD_BWD / fb / 1e9 / HBM_TBS, 5))
    return res


def step_eager(name, reps):
    import torch
    shape = SHAPES[name]
    ps = pairs(shape, 2)
    n = len(ps)
    loss = lambda a, b: ((eager_mind(a) - eager_mind(b)) ** 2).mean()
    with torch.no_grad():
        fwd = median_ms(lambda i: loss(*ps[i % n]), reps, warm=2)
    both = median_ms(lambda i: torch.autograd.grad(loss(*ps[i % n]), ps[i % n]), reps, warm=2)
    return {"eager": {"fwd_ms": round(fwd, 3), "fwd_bwd_ms": round(both, 3)}}


def step_model(similarity, reps):
    import torch
    from dfmir_amd.registration3d import Registration3DModel
    shape = SHAPES["128x128x128"]
    torch.manual_seed(0)
    A = torch.rand(1, 1, *shape, device=DEV)
    B = 0.5 * A + 0.5 * torch.rand(1, 1, *shape, device=DEV)
    m = Registration3DModel(shape, device=DEV, capture_step=True, similarity=similarity)

    def step(i):
        m.set_input({"A": A, "B": B})
        m.optimize_parameters()
    ms = median_ms(step, reps, warm=5)
    assert m._graph['graph'] is not None
    return {"captured_step_%s_ms" % similarity: round(ms, 4)}


STEPS = [("kernels", "160x192x224", 240), ("kernels", "128x128x128", 180), ("eager", "160x192x224", 240),
         ("eager", "128x128x128", 180), ("model", "ncc", 240), ("model", "mind", 240)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=2, default=None, help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        kind, arg = args.step
        fn = {"kernels": step_kernels, "eager": step_eager, "model": step_model}[kind]
        print("RESULT " + json.dumps(fn(arg, args.reps if kind != "eager" else max(3, args.reps // 4))), flush=True)
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
        r = json.loads(line[7:])
        res.setdefault(arg if kind != "model" else "128x128x128", {}).update(r)
        print("%-8s %-12s %s" % (kind, arg, json.dumps(r)), flush=True)
    st = res["128x128x128"]
    st["captured_step_mind_over_ncc"] = round(st["captured_step_mind_ms"] / st["captured_step_ncc_ms"], 3)
    print("128^3 captured step: mind / ncc = %.3f" % st["captured_step_mind_over_ncc"], flush=True)
    if args.out:
        import torch
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "hbm_tbs": HBM_TBS, "result": res}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
