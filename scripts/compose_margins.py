"""The yardstick of tests/test_compose.py: how far the definitions of ops.compose_flows and ops.invert_flow evaluated by torch
in fp32 on the CPU lie from the float64 restatement, per case of the test's set and per input family, and -- when a HIP device
is present -- how far the kernels lie.  profiles/compose_margins.txt records the output; the test's bounds are 4x the maxima of
the fp32 CPU columns (rows "max"), per family and quantity, and its residual floors 4x the "floor" rows (the fp32 CPU evaluation's statistics after the last iteration).  The du columns leave
out what the test leaves out (smooth family: voxels with a sample coordinate within 1e-4 of an integer).

    python scripts/compose_margins.py            # CPU columns only without a device
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_compose as T  # noqa: E402

F32 = torch.float32


def fmt(name, tag, r):
    print("%-21s %-9s | %s" % (name, tag, "  ".join("%.2e" % x for x in r)))


def worst_of(rows):
    return [max(col) for col in zip(*rows)]


def floors(hist):
    """where a history ends: the statistics of the last iteration, the largest over the samples, (rms, max)"""
    return tuple(float(hist[-1, :, c].max()) for c in (0, 1))


def main():
    gpu = torch.cuda.is_available()
    side = lambda cols: "fp32 CPU: %s%s" % (cols, " | kernels: " + cols if gpu else "")

    print("compose_flows         family    | " + side("val-l2  val-max  du-l2  du-max  dv-l2  dv-max"))
    for fam in T.FAMILIES:
        rows = []
        for shape in T.SHAPES:
            u, v, g, ref, keep = T.compose_reference(shape, fam)
            r = list(T.compose_errors(T.compose_ref(u, v, g, dtype=F32), ref, keep))
            if gpu:
                r += list(T.compose_errors(T._gpu_compose(u, v, g), ref, keep))
            rows.append(r)
            fmt(T._id(shape), fam, r)
        fmt("max", fam, worst_of(rows))

    print("\ninvert_flow, 1 step   family    | " + side("w-l2  w-max  rms_0  max_0  rms_1  max_1"))
    rows = []
    for shape in T.SHAPES:
        u, init, (w64, h64) = T.step_reference(shape)
        err = lambda w, h: list(T.field_errors(w, w64) + T.stat_errors(h[0], h64[0]) + T.stat_errors(h[1], h64[1]))
        r = err(*T.invert_ref(u, 1, init=init, dtype=F32))
        if gpu:
            r += err(*T._gpu_invert(u, iters=1, init=init, history=True))
        rows.append(r)
        fmt(T._id(shape), "lattice", r)
    fmt("max", "lattice", worst_of(rows))

    print("\ninvert_flow, %d iters family    | %s" % (T.ITERS, side("w-l2  w-max  hist-rms  hist-max")))
    rows = []
    for shape in T.WINDOWED:
        u, (w64, h64) = T.windowed_reference(shape)
        w32, h32 = T.invert_ref(u, T.ITERS, dtype=F32)
        fl = floors(h32)
        floor = tuple(T.FACTOR * x for x in fl)
        err = lambda w, h: list(T.field_errors(w, w64) + T.history_errors(h, h64, floor))
        r = err(w32, h32)
        extra = "fp64 rms_20 %.1e" % float(h64[-1, :, 0].max())
        if gpu:
            wg, hg = T._gpu_invert(u, iters=T.ITERS, history=True)
            r += err(wg, hg)
            extra += "; kernels' last (rms, max) %.2e %.2e" % floors(hg)
        rows.append(r)
        fmt(T._id(shape), "windowed", r)
        print("%-21s %-9s | %.2e  %.2e   (fp32 CPU rms_%d, max_%d; %s)" % (T._id(shape), "floor", fl[0], fl[1], T.ITERS, T.ITERS, extra))
    fmt("max", "windowed", worst_of(rows))

    shape = T.WINDOWED[0]
    lab = T.label_blocks(shape[2:])
    u, (w64, _) = T.windowed_reference(shape)
    want = T.nearest_pull(lab, w64)
    share = float((T.nearest_pull(lab, T.invert_ref(u, T.ITERS, dtype=F32)[0]) != want).float().mean())
    line = "\npull_back_label %s: the fp32 CPU evaluation flips %.3e of the voxels' labels" % (T._id(shape), share)
    if gpu:
        from dfmir_amd import infer
        out = infer.pull_back_label(lab.to(T.DEV), u.to(T.DEV), iters=T.ITERS)
        line += "; the kernels %.3e" % float((out["label"].cpu() != want).float().mean())
    print(line + " (%d voxels, %.3f of them change label under the flow)" % (lab.numel(), float((want != lab).float().mean())))

    (moving, fixed, flow0), (flow64, hist64, _) = T.refine_reference()
    r = list(T.field_errors(T.refine_compose_ref(moving, fixed, flow0, dtype=F32, **T.REFINE_KW)[0], flow64))
    if gpu:
        from dfmir_amd import infer
        out = infer.refine_flow(moving.to(T.DEV), fixed.to(T.DEV), flow0.to(T.DEV), features='intensity', update='compose',
                                **T.REFINE_KW)
        r += list(T.field_errors(out["flow"], flow64))
    print("\nrefine_flow(update='compose'), %d iterations at %s | %s" % (T.REFINE_KW["iters"], T._id(T.REFINE_VOL),
                                                                         side("flow-l2  flow-max")))
    fmt("max", "refine", r)


if __name__ == "__main__":
    main()
