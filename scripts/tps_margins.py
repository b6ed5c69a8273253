"""profiles/tps_margins.txt: per case of tests/test_tps.py the error e32 of the thin-plate-spline definition evaluated by
torch in fp32 on the CPU (coefficients rounded to fp32) against the float64 restatement, the bound the tests derive from it
(4 e32 + 4 * 2^-23 max|u|; relative 2-norm for dcoef) and -- with a GPU -- the kernels' own errors beside them.

    python scripts/tps_margins.py [--out profiles/tps_margins.txt]

The CPU columns need no GPU; without one the kernel columns read "-"."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from dfmir_amd import ops  # noqa: E402
from tests import test_tps as T  # noqa: E402

WHAT = ('flow', 'ctrl', 'rand', 'dcoef')


def kernel_errors(case, r):
    fit = T.gpu_fit(r)
    coef = r.coef.to(T.DEV).requires_grad_()
    flow = ops.tps_flow(coef, handle=fit)
    dcoef, = torch.autograd.grad(flow, coef, r.g.to(T.DEV))
    full = ops.tps_flow(fit)                                   # through the device's own solve
    return {
        'flow': float((full.double().cpu() - r.flow).abs().max()),
        'ctrl': float((ops.tps_points(fit, fit.ctrl).double().cpu() - r.at_ctrl).abs().max()),
        'rand': float((ops.tps_points(fit, r.rand.to(T.DEV)).double().cpu() - r.at_rand).abs().max()),
        'dcoef': float((dcoef.cpu() - r.dcoef).norm() / r.dcoef.norm()),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tps_margins.txt"))
    args = ap.parse_args()
    gpu = torch.cuda.is_available()
    lines = ["# thin-plate-spline kernels (dfmir_amd/csrc/tps.hip) against the float64 restatement of tests/test_tps.py",
             "# e32 = the same definition in fp32 on the CPU; bound = 4 e32 + 4 * 2^-23 max|u| (dcoef: relative 2-norm);",
             "# kernel = ops.tps_flow / ops.tps_points / dcoef on %s" % (torch.cuda.get_device_name(0) if gpu else "- (no GPU)"),
             "# flow, ctrl (the spline at its control points), rand (at random points): max-abs, voxels",
             "%-46s %-6s %10s %10s %10s %8s" % ("case", "what", "e32", "bound", "kernel", "k/bound")]
    worst = 0.0
    for case in T.CASES:
        r = T.reference(case)
        k = kernel_errors(case, r) if gpu else {}
        for w in WHAT:
            ke = k.get(w)
            if ke is not None:
                worst = max(worst, ke / r.bound[w])
            lines.append("%-46s %-6s %10.3e %10.3e %10s %8s" % (
                T._id(case), w, r.e32[w], r.bound[w], "-" if ke is None else "%.3e" % ke,
                "-" if ke is None else "%.3f" % (ke / r.bound[w])))
        print(lines[-4], flush=True)
    if gpu:
        lines.append("# worst kernel / bound: %.3f" % worst)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
