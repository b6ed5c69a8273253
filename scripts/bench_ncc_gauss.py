"""GPU box: NCC_Loss forward + backward with the 'mean' (win 9) and the 'gaussian' (sigma 3) window at [16,1,256,256] and
[1,1,160,192,224], and Registration3DModel steps at 128^3 with each.  HIP-event timed, one event pair per call, medians;
the inputs rotate over enough pairs to exceed the 256 MB Infinity Cache, so every call reads them from HBM.  The HBM
fraction sets the floats the launches move as implemented (2-D: forward 12 N, backward 14 N; 3-D: 22 N and 14 N; N = voxels)
against 6.3 TB/s, the achievable rate of a float4 copy.

    python scripts/bench_ncc_gauss.py [--kernels mean,gaussian] [--repo DIR] [--reps 30] [--out FILE]

--repo DIR imports dfmir_amd from another checkout (with its own built library): the parent commit's 'mean' rows.
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--kernels", default="mean,gaussian")
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.repo))

import torch                                              # noqa: E402

from dfmir_amd.losses import NCC_Loss                     # noqa: E402
from dfmir_amd.registration3d import Registration3DModel  # noqa: E402

DEV = "cuda"
HBM_TBS = 6.3


def median_ms(fn, reps, warm=5):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (s, e) in enumerate(ev):
        s.record()
        fn(warm + i)
        e.record()
    torch.cuda.synchronize()
    t = sorted(s.elapsed_time(e) for s, e in ev)
    return statistics.median(t), t[0], t[-1]


def loss_rows(kernel):
    rows = []
    for shape in ((16, 1, 256, 256), (1, 1, 160, 192, 224)):
        nd = len(shape) - 2
        N = 1
        for s in shape:
            N *= s
        npairs = max(3, -(-(512 << 20) // (8 * N)))
        Js = [torch.rand(*shape, device=DEV) for _ in range(npairs)]
        Is = [(0.6 * torch.rand_like(j) + 0.4 * j).requires_grad_() for j in Js]
        crit = NCC_Loss(DEV, kernel_type=kernel) if kernel == 'gaussian' else NCC_Loss(DEV, kernel_var=[9] * nd)

        def fwd_bwd(i):
            x = Is[i % npairs]
            x.grad = None
            crit(x, Js[i % npairs]).backward()

        def fwd(i):
            with torch.no_grad():
                crit(Is[i % npairs], Js[i % npairs])

        both, lo, hi = median_ms(fwd_bwd, args.reps)
        f, _, _ = median_ms(fwd, args.reps)
        floats = (12 + 14) * N if nd == 2 else (22 + 14) * N
        frac = 4.0 * floats / (both * 1e-3) / (HBM_TBS * 1e12)
        rows.append({"what": "loss", "kernel": kernel, "shape": list(shape), "fwd_bwd_ms": round(both, 4), "min_ms": round(lo, 4),
                     "max_ms": round(hi, 4), "fwd_ms": round(f, 4), "hbm_fraction_fwd_bwd": round(frac, 3)})
        print("%-8s loss %-18s fwd+bwd %7.3f ms (min %.3f max %.3f)  fwd %7.3f ms  %4.1f %% of %.1f TB/s" %
              (kernel, "x".join(map(str, shape)), both, lo, hi, f, 100 * frac, HBM_TBS), flush=True)
        del Is, Js
        torch.cuda.empty_cache()
    return rows


def step_row(kernel):
    shape = (128, 128, 128)
    torch.manual_seed(0)
    kw = {"ncc_kernel": kernel} if kernel == 'gaussian' else {}
    m = Registration3DModel(shape, None, device=DEV, capture_step=True, **kw)
    data = []
    for i in range(4):
        A = torch.rand(1, 1, *shape, device=DEV)
        data.append({"A": A, "B": 0.5 * A + 0.5 * torch.rand_like(A)})
    for i in range(6):
        m.set_input(data[i % 4]); m.optimize_parameters()
    torch.cuda.synchronize()
    t = []
    for i in range(args.steps):
        t0 = time.perf_counter()
        m.set_input(data[i % 4]); m.optimize_parameters()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(t)
    print("%-8s Registration3DModel 128^3 captured step %7.3f ms (min %.3f max %.3f)  ncc %.5f" %
          (kernel, med, min(t), max(t), m.get_current_losses()["ncc"]), flush=True)
    return {"what": "step128", "kernel": kernel, "step_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}


def main():
    rows = []
    for kernel in args.kernels.split(","):
        rows += loss_rows(kernel)
        rows.append(step_row(kernel))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
