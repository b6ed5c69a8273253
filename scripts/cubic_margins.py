"""The yardstick of tests/test_cubic.py: how far the cubic B-spline definitions evaluated by torch in fp32 on the CPU lie from the
float64 restatement, per case of the test's set -- ops.spline_prefilter (relative 2-norm and max-abs over max, per shape),
ops.warp_cubic forward and d(flow) (the same two measures, per shape and flow kind) -- and, when a HIP device is present, how
far the kernels lie.  The test's bounds are 4x the maxima of the fp32 columns, over the small shapes and over the large ones
separately.  The fp32 figures depend on the host's thread count; profiles/ keeps a run on a host with the device
(cubic_margins.txt) and one on a host without (cubic_margins_cpu.txt), and the test quotes the smaller figure per quantity.

    python scripts/cubic_margins.py [out.txt]    # default profiles/cubic_margins.txt with a device, cubic_margins_cpu.txt without
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import test_cubic as T  # noqa: E402

COLS = ("l2", "max")


def main():
    gpu = torch.cuda.is_available()
    default = os.path.join(REPO, "profiles", "cubic_margins.txt" if gpu else "cubic_margins_cpu.txt")
    path = sys.argv[1] if len(sys.argv) > 1 else default
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    heads = ["fp32 CPU"] + (["kernels"] if gpu else [])
    worst = {}

    def row(what, grp, label, groups):
        emit("%-34s | %s" % (label, " | ".join("  ".join("%.2e" % g[c] for c in COLS) for g in groups)))
        for i, g in enumerate(groups):
            for c in COLS:
                worst[(what, grp, i, c)] = max(worst.get((what, grp, i, c), 0.0), g[c])

    emit("spline_prefilter: " + "  ".join(COLS) + "      (" + " | ".join(heads) + ")")
    for shape in T.PREFILTER_SHAPES + [T.STRIDED_SHAPE]:
        x = T.image(shape)
        ref = T.prefilter_ref(x)
        groups = [T.field_errors(T.prefilter_ref(x, torch.float32), ref)]
        if gpu:
            groups.append(T.field_errors(T._gpu_prefilter(x), ref))
        row("prefilter", T.group_of(shape), T._id(shape), groups)
    emit()
    emit("warp_cubic, forward then d(flow): " + "  ".join(COLS) + "      (" + " | ".join(heads) + ")")
    for shape in T.WARP_SHAPES:
        for kind in T.KINDS:
            (src, flow, dout), (ref_out, ref_g) = T.warp_reference(shape, kind)
            out32, g32 = T.warp_cubic_ref_grad(src, flow, dout, torch.float32)
            fwd, bwd = [T.field_errors(out32, ref_out)], [T.field_errors(g32, ref_g)]
            if gpu:
                out, g = T._gpu_warp(src, flow, dout)
                fwd.append(T.field_errors(out, ref_out))
                bwd.append(T.field_errors(g, ref_g))
            row("forward", T.group_of(shape), "%-14s %-8s forward" % (T._id(shape), kind), fwd)
            row("dflow", T.group_of(shape), "%-14s %-8s d(flow)" % (T._id(shape), kind), bwd)
    emit()
    for what in ("prefilter", "forward", "dflow"):
        for grp in ("small", "large"):
            for i, h in enumerate(heads):
                if (what, grp, i, COLS[0]) in worst:
                    emit("max, %-9s %-5s %-9s: " % (what, grp, h) + "  ".join("%s %.2e" % (c, worst[(what, grp, i, c)]) for c in COLS))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
