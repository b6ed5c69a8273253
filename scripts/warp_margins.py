"""The yardstick of tests/test_gpu_warp_fp64.py: how far the definitions of ops.warp, ops.vecint_step and the seven-step
integration evaluated by torch in fp32 on the CPU (tests/ref64.py with dtype=float32) lie from the float64 restatement, per
case of the test's set and per input family, and -- when a HIP device is present -- how far the kernels lie (informative only:
the test's bounds are 4x the rows "max" of the fp32 CPU columns).  The d(flow) and dv columns leave out what the test leaves
out (smooth families: voxels with a sample coordinate within 1e-4 of an integer).  The resize bounds are computed per case
inside the test; their table is printed last.

    python scripts/warp_margins.py [out]         # writes profiles/warp_margins.txt; CPU columns only without a device
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_gpu_warp_fp64 as W  # noqa: E402

F32 = torch.float32
LINES = []


def say(line=""):
    print(line)
    LINES.append(line)


def fmt(op, name, tag, r, n):
    cols = ["  ".join("%.2e" % x for x in r[i:i + n]) for i in range(0, len(r), n)]
    say("%-7s %-22s %-9s | %s" % (op, name, tag, " | ".join(cols)))


def worst_of(rows):
    return [max(col) for col in zip(*rows)]


def main():
    gpu = torch.cuda.is_available()
    side = lambda cols: "fp32 CPU: %s%s" % (cols, " | kernels: " + cols if gpu else "")

    say("op      case                   family   | " + side("val-l2  val-max  dsrc-l2  dsrc-max  dflow-l2  dflow-max")
        + ("  (both gradients; then flow only: dflow; src only: dsrc; windowed shapes: ops._warp_bwd dsrc, dflow)" if gpu else ""))
    for fam in W.WARP_FAMILIES:
        rows = []
        for shape in W.SHAPES:
            src, flow, g, ref, keep = W.warp_case(shape, fam)
            r = list(W.warp_errors(W.warp_eval(src, flow, g, dtype=F32), ref, keep))
            if gpu:
                r += list(W.warp_errors(W.gpu_warp(src, flow, g), ref, keep))
            rows.append(r)
            fmt("warp", W._id(shape), fam, r, 6)
            if gpu:
                extra = list(W.rel_errors(W.gpu_warp(src, flow, g, want_src=False)[2], ref[2], keep))
                extra += list(W.rel_errors(W.gpu_warp(src, flow, g, want_flow=False)[1], ref[1]))
                if shape[-1] % 4 == 0:
                    dsrc, dflow = W.gpu_warp_atomic(src, flow, g)
                    extra += list(W.rel_errors(dsrc, ref[1]) + W.rel_errors(dflow, ref[2], keep))
                say("%-7s %-22s %-9s   other backward forms: %s" % ("", "", "", "  ".join("%.2e" % x for x in extra)))
        fmt("warp", "max", fam, worst_of(rows), 6)

    say()
    say("op      case                   family   | " + side("val-l2  val-max  dv-l2  dv-max"))
    for fam in W.VI_FAMILIES:
        rows = []
        for shape in W.VI_SHAPES:
            v, g, ref, keep = W.vecint_case(shape, fam)
            r = list(W.vecint_errors(W.vecint_eval(v, g, dtype=F32), ref, keep))
            if gpu:
                r += list(W.vecint_errors(W.gpu_vecint(v, g), ref, keep))
            rows.append(r)
            fmt("vecint", W._id(shape), fam, r, 4)
        fmt("vecint", "max", fam, worst_of(rows), 4)

    say()
    say("op      case                   family   | " + side("val-l2  val-max  dv-l2  dv-max")
        + "   (%d steps behind the 1 / 128 scale)" % W.CHAIN_STEPS)
    for fam in W.CHAIN_FAMILIES:
        rows = []
        for shape in W.CHAIN_SHAPES:
            v, g, ref, coords = W.chain_case(shape, fam)
            r = list(W.vecint_errors(W.vecint_eval(v, g, dtype=F32, steps=W.CHAIN_STEPS, pre=1.0 / 128), ref, None))
            if gpu:
                r += list(W.vecint_errors(W.gpu_vecint(v, g, steps=W.CHAIN_STEPS, pre=1.0 / 128), ref, None))
            rows.append(r)
            fmt("chain", W._id(shape), fam, r, 4)
        fmt("chain", "max", fam, worst_of(rows), 4)

    say()
    say("resize  case                   mult     | bound: value  dx" + (" | kernels: value-max  dx-max" if gpu else "")
        + "   (bound = max(16 x 2^-24, 4 x fp32 F.interpolate on the CPU), of the maximum)")
    for case in W.RESIZE_CASES:
        for mult in W.RESIZE_MULTS:
            x, cot, ref, bounds = W.resize_case(case, mult)
            r = list(bounds)
            if gpu:
                got = W.gpu_resize(x, cot, case[1], mult)
                r += [W.rel_errors(got[0], ref[0])[1], W.rel_errors(got[1], ref[1])[1]]
            fmt("resize", W._rid(case), "%g" % mult, r, 2)

    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "warp_margins.txt")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
