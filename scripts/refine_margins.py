"""The yardstick of tests/test_refine.py: how far the warped-feature SSD evaluated by torch in fp32 on the CPU lies from the
float64 restatement, per case of the test's set (shape, input family, mask), and -- when a HIP device is present -- how far the
kernels lie on the packed and on the planar path; then the same for the final similarity of the 40-iteration refinement loop
(fp32 CPU loop against the float64 loop, and infer.refine_flow against it).  profiles/refine_margins.txt records the output;
the test's bounds are 4x the maxima of the fp32 columns, per family, and 4x the fp32 gap of the loop.

    python scripts/refine_margins.py            # CPU columns only without a device
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_refine as T  # noqa: E402

COLS = "loss  L_b  dflow-l2  dflow-max"


def fmt(name, fam, mask, groups):
    cell = lambda x: "   -    " if x is None else "%.2e" % x
    print("%-14s %-8s %-8s | %s" % (name, fam, mask, " | ".join("  ".join(cell(x) for x in g) for g in groups)))


def main():
    gpu = torch.cuda.is_available()
    heads = ["fp32 CPU: " + COLS] + (["kernels, packed: " + COLS, "kernels, planar: " + COLS] if gpu else [])
    print("case           family   mask     | " + " | ".join(heads))
    worst = {}
    for shape in T.SHAPES:
        for fam in T.FAMILIES:
            for mask in ("none", "partial"):
                inp, ref = T.reference(shape, fam, mask)
                vo = fam == "integer"
                groups = [T.errors(T.ssd_ref(*inp, dtype=torch.float32), ref, vo)]
                if gpu:
                    groups += [T.errors(T._gpu(*inp, path=p), ref, vo) for p in T.PATHS]
                fmt(T._id(shape), fam, mask, groups)
                w = worst.setdefault(fam, [[0.0] * 4 for _ in groups])
                for g, wg in zip(groups, w):
                    for i, x in enumerate(g):
                        wg[i] = None if x is None else max(wg[i], x)
    for fam in T.FAMILIES:
        fmt("max", fam, "", worst[fam])

    print()
    print("refinement loop %s, %s" % (T.REFINE_VOL, T.REFINE_KW))
    (moving, fixed, true), (flow64, h64) = T.refine_reference()
    flow32, h32 = T.refine_ref(moving, fixed, dtype=torch.float32, **T.REFINE_KW)
    zero = torch.zeros_like(true)
    line = lambda name, h, flow: print("%-18s similarity %.6e -> %.6e   regulariser %.4e   flow error %.4f -> %.4f   "
                                       "final similarity against fp64: %.3e"
                                       % (name, float(h[0, 0]), float(h[-1, 0]), float(h[-1, 1]), T.flow_error(zero, true),
                                          T.flow_error(flow, true), abs(float(h[-1, 0]) - float(h64[-1, 0])) / float(h64[-1, 0])))
    line("fp64 CPU loop", h64, flow64)
    line("fp32 CPU loop", h32, flow32)
    if gpu:
        from dfmir_amd import _lib, infer
        for path in T.PATHS:
            with T.planar_path(path):
                out = infer.refine_flow(moving.to(T.DEV), fixed.to(T.DEV), features='intensity', **T.REFINE_KW)
                line("refine_flow, " + path, out['history'].cpu().double(), out['flow'])


if __name__ == "__main__":
    main()
