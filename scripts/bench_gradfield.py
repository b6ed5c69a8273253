"""GPU box: the normalised-gradient-field loss (dfmir_amd.ops.gradfield_loss, csrc/gradfield.hip), forward + backward with
gradients to both images, at 160x192x224, 128^3 and a 2-D 256^2 batch of 16: beside the same definition composed from eager
torch ops on the same GPU (replicate padding and slicing), and beside ops.mind_loss and the box ops.ncc_loss on the same
tensors; and a captured 128^3 Registration3DModel step with similarity='gradfield' against 'ncc' and 'mind'.  HIP-event
timed per call, medians over `--reps` calls after a warm-up, over a rotating set of image pairs larger than the 256 MiB
Infinity Cache, so every call reads its inputs from HBM.

Every step runs in a child process of its own under its own time limit; a step that fails or runs out of time ends the
run (no retries).

    python scripts/bench_gradfield.py [--reps 20] [--out profiles/gradfield_bench.json]
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
SHAPES = {"160x192x224": (1, 160, 192, 224), "128x128x128": (1, 128, 128, 128), "16x256x256": (16, 256, 256)}
ROTATE_BYTES = 384 << 20           # the rotating inputs together exceed the 256 MiB Infinity Cache
# Bytes per voxel (fp32, halo re-reads not counted).  eps='auto': the statistics pass reads both images (8), the loss pass
# reads them again (8), the backward reads them a third time and writes both gradients (8 + 8).  A given eps saves the
# first 8.  No intermediate volume exists, so this is also the algorithmic traffic of the definition with 'auto'.
BYTES_FWD, BYTES_FWD_BWD = 16, 32


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


def batch_shape(name):
    s = SHAPES[name]
    return (s[0], 1) + tuple(s[1:])


def pairs(name):
    import torch
    shape = batch_shape(name)
    vox = 1
    for v in shape:
        vox *= v
    n = max(2, -(-ROTATE_BYTES // (8 * vox)))
    g = torch.Generator(device=DEV).manual_seed(1)
    out = []
    for _ in range(n):
        a = torch.rand(*shape, device=DEV, generator=g)
        b = 0.5 * a + 0.5 * torch.rand(*shape, device=DEV, generator=g)
        out.append((a.requires_grad_(), b.requires_grad_()))
    return out, vox


def eager_gradfield(a, b, eta=1.0):
    """The definition (eps='auto', unit spacing) from stock torch ops: the composition the tree could run without the kernels."""
    import torch
    import torch.nn.functional as F
    nd = a.dim() - 2

    def grads(I):
        P = F.pad(I, (1, 1) * nd, mode='replicate')
        out = []
        for ax in range(nd):
            hi = [slice(None), slice(None)] + [slice(1, 1 + n) for n in I.shape[2:]]
            lo = list(hi)
            hi[2 + ax] = slice(2, 2 + I.shape[2 + ax])
            lo[2 + ax] = slice(0, I.shape[2 + ax])
            out.append((P[tuple(hi)] - P[tuple(lo)]) * 0.5)
        return out

    ga, gb = grads(a), grads(b)
    na, nb = sum(g * g for g in ga), sum(g * g for g in gb)
    ea, eb = eta * na.detach().sqrt().mean(), eta * nb.detach().sqrt().mean()
    dot = sum(p * q for p, q in zip(ga, gb))
    return (1.0 - dot * dot / ((na + ea * ea) * (nb + eb * eb))).mean()


def step_kernels(name, reps):
    import torch
    from dfmir_amd import ops
    ps, vox = pairs(name)
    n = len(ps)
    res = {"rotating_pairs": n}
    for tag, fn, both in (("gradfield", lambda a, b: ops.gradfield_loss(a, b), True),
                          ("gradfield_given_eps", lambda a, b: ops.gradfield_loss(a, b, eps=(0.05, 0.05)), True),
                          ("mind", lambda a, b: ops.mind_loss(a, b), True),
                          ("ncc_box", lambda a, b: ops.ncc_loss(a, b, 9), False)):
        with torch.no_grad():
            fwd = median_ms(lambda i: fn(*ps[i % n]), reps)
        fb = median_ms(lambda i: torch.autograd.grad(fn(*ps[i % n]), ps[i % n][:2 if both else 1]), reps)
        res[tag] = {"fwd_ms": round(fwd, 4), "fwd_bwd_ms": round(fb, 4)}
    for tag, saved in (("gradfield", 0), ("gradfield_given_eps", 8)):
        r = res[tag]
        r.update(fwd_bytes_per_voxel=BYTES_FWD - saved, fwd_bwd_bytes_per_voxel=BYTES_FWD_BWD - saved,
                 fwd_tbs=round(vox * (BYTES_FWD - saved) / r["fwd_ms"] / 1e9, 3),
                 fwd_bwd_tbs=round(vox * (BYTES_FWD_BWD - saved) / r["fwd_bwd_ms"] / 1e9, 3))
        r.update(fwd_hbm_frac=round(r["fwd_tbs"] / HBM_TBS, 4), fwd_bwd_hbm_frac=round(r["fwd_bwd_tbs"] / HBM_TBS, 4))
    return res


def step_eager(name, reps):
    import torch
    ps, _ = pairs(name)
    n = len(ps)
    with torch.no_grad():
        fwd = median_ms(lambda i: eager_gradfield(*ps[i % n]), reps, warm=2)
    fb = median_ms(lambda i: torch.autograd.grad(eager_gradfield(*ps[i % n]), ps[i % n]), reps, warm=2)
    return {"eager": {"fwd_ms": round(fwd, 3), "fwd_bwd_ms": round(fb, 3)}}


def step_model(similarity, reps):
    import torch
    from dfmir_amd.registration3d import Registration3DModel
    shape = SHAPES["128x128x128"][1:]
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


STEPS = [("kernels", n, 240) for n in SHAPES] + [("eager", n, 240) for n in SHAPES] + \
        [("model", s, 240) for s in ("ncc", "mind", "gradfield")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=2, default=None, help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        kind, arg = args.step
        fn = {"kernels": step_kernels, "eager": step_eager, "model": step_model}[kind]
        print("RESULT " + json.dumps(fn(arg, args.reps if kind != "eager" else max(5, args.reps // 2))), flush=True)
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
    ok = True
    for name in SHAPES:
        k, e = res[name]["gradfield"]["fwd_bwd_ms"], res[name]["eager"]["fwd_bwd_ms"]
        res[name]["eager_over_gradfield"] = round(e / k, 2)
        print("%s: forward + backward %.4f ms, eager %.3f ms: %.1fx%s" % (name, k, e, e / k, "" if k < e else "  ** NOT FASTER **"),
              flush=True)
        ok = ok and k < e
    st = res["128x128x128"]
    g, n, m = (st["captured_step_%s_ms" % s] for s in ("gradfield", "ncc", "mind"))
    print("128^3 captured step: ncc %.4f ms, mind %.4f ms, gradfield %.4f ms%s" % (n, m, g, "" if g <= m else "  ** SLOWER THAN MIND **"),
          flush=True)
    res["acceptance"] = {"kernels_beat_eager": ok, "step_not_slower_than_mind": g <= m}
    if args.out:
        import torch
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "hbm_tbs": HBM_TBS, "result": res}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
