"""The yardstick of tests/test_bspline.py: how far the cubic B-spline expansion (the gather form of the definition) evaluated by
torch in fp32 on the CPU lies from the float64 restatement, forward and adjoint, per case of the test's set, and -- when a HIP
device is present -- how far ops.bspline_flow's kernels lie; then the same for the final similarity of the 40-iteration
refinement loop at control spacing 4 (fp32 CPU loop against the float64 loop, and infer.refine_flow(parametrisation='bspline')
against it), with the linear loop at the same spacing beside it.  profiles/bspline_margins.txt records the output; the test's
bounds are 4x the row "max" of the fp32 columns and 4x the fp32 gap of the loop.

    python scripts/bspline_margins.py           # CPU columns only without a device
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_bspline as T  # noqa: E402
from tests import test_refine as R  # noqa: E402

COLS = "fwd-max  fwd-l2   adj-max  adj-l2"


def fmt(name, groups):
    print("%-22s | %s" % (name, " | ".join("  ".join("%.2e" % x for x in g) for g in groups)))


def main():
    gpu = torch.cuda.is_available()
    print("case                   | " + " | ".join(["fp32 CPU: " + COLS] + (["kernels:  " + COLS] if gpu else [])))
    worst = None
    for case in T.CASES:
        (ctrl, dy), (y64, g64) = T.reference(case)
        y32, g32 = T.evaluate(case, ctrl, dy, torch.float32)
        groups = [T.errors(y32, y64) + T.errors(g32, g64)]
        if gpu:
            y, g = T._gpu(case, ctrl, dy)
            groups.append(T.errors(y, y64) + T.errors(g, g64))
        fmt(T._id(case), groups)
        worst = groups if worst is None else [tuple(max(a, b) for a, b in zip(w, g)) for w, g in zip(worst, groups)]
    fmt("max", worst)

    print()
    print("refinement loop %s, %s" % (R.REFINE_VOL, T.BSPLINE_KW))
    (moving, fixed, true), (flow64, h64) = T.refine_reference()
    flow32, h32 = T.bspline_refine_ref(moving, fixed, dtype=torch.float32, **T.BSPLINE_KW)
    lin64, hl64 = R.refine_ref(moving, fixed, **T.BSPLINE_KW)
    zero = torch.zeros_like(true)

    def line(name, h, flow, ref):
        print("%-28s similarity %.6e -> %.6e   regulariser %.4e   flow error %.4f -> %.4f   final similarity against "
              "its fp64 loop: %.3e" % (name, float(h[0, 0]), float(h[-1, 0]), float(h[-1, 1]), R.flow_error(zero, true),
                                       R.flow_error(flow, true), abs(float(h[-1, 0]) - float(ref[-1, 0])) / float(ref[-1, 0])))

    line("B-spline, fp64 CPU loop", h64, flow64, h64)
    line("B-spline, fp32 CPU loop", h32, flow32, h64)
    line("linear, fp64 CPU loop", hl64, lin64, hl64)
    if gpu:
        from dfmir_amd import infer
        mv, fx = moving.to(T.DEV), fixed.to(T.DEV)
        out = infer.refine_flow(mv, fx, features='intensity', parametrisation='bspline', **T.BSPLINE_KW)
        line("refine_flow, 'bspline'", out['history'].cpu().double(), out['flow'], h64)
        out = infer.refine_flow(mv, fx, features='intensity', **T.BSPLINE_KW)
        line("refine_flow, 'linear'", out['history'].cpu().double(), out['flow'], hl64)


if __name__ == "__main__":
    main()
