"""The yardstick of tests/test_affine.py: how far the affine definitions evaluated by torch in fp32 on the CPU lie from the
float64 restatement, per case of the test's set (shape, theta kind, mask) -- the flow (absolute) and its adjoint, the value and
L_b (relative), gb = dL/dtheta, g and H (relative 2-norm and max-abs over max) -- and, when a HIP device is present, how far the
kernels lie; then the theta the Levenberg-Marquardt loop ends at on the two recovery fixtures: the fp32 CPU restatement of the
whole loop (system in fp32, solve in float64, theta kept in fp32) against the float64 loop, and infer.affine_init against it.
The test's bounds are 4x the maxima of the fp32 columns -- taken over the five small shapes and over the one large shape
separately, since fp32 coordinates of a thousand voxels carry another error than those of ten -- and 4x the fp32 gap of the loop.
The fp32 figures depend on the host's thread count; profiles/ keeps a run on a host with the device (affine_margins.txt) and one
on a host without (affine_margins_cpu.txt), and the test quotes the smaller figure per quantity.

    python scripts/affine_margins.py [out.txt]       # default profiles/affine_margins.txt; CPU columns only without a device
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import test_affine as T  # noqa: E402

FLOW_COLS = ("flow", "dtheta_l2", "dtheta_max")
SYS_COLS = ("L", "Lb", "gb_l2", "gb_max", "g_l2", "g_max", "H_l2", "H_max")


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "affine_margins.txt")
    lines = []

    def emit(s=""):
        print(s)
        lines.append(s)

    gpu = torch.cuda.is_available()
    worst = {}

    def row(name, kind, mask, cols, groups):
        emit("%-16s %-9s %-8s | %s" % (name, kind, mask, " | ".join("  ".join("%.2e" % g[c] for c in cols) for g in groups)))
        for i, g in enumerate(groups):
            for c in cols:
                key = (T.group_of(tuple(int(v) for v in name.split("x"))), i, c)
                worst[key] = max(worst.get(key, 0.0), g[c])

    heads = ["fp32 CPU"] + (["kernels"] if gpu else [])
    emit("affine_flow and its adjoint: " + "  ".join(FLOW_COLS) + "      (" + " | ".join(heads) + ")")
    for shape in T.SHAPES:
        for kind in T.KINDS:
            theta = T.thetas(shape, kind, 1300 + 19 * T.SHAPES.index(shape) + 7)
            vol = tuple(shape[2:])
            groups = [T.flow_errors(T.affine_flow_ref(theta, vol), T.affine_flow_adjoint_ref(T.dflow_of(shape)), theta, shape)]
            if gpu:
                groups.append(T.flow_errors(*T._gpu_flow(theta, shape), theta, shape))
            row(T._id(shape), kind, "", FLOW_COLS, groups)
    emit()
    emit("affine_ssd / affine_ssd_system: " + "  ".join(SYS_COLS) + "      (" + " | ".join(heads) + ")")
    for shape in T.SHAPES:
        for kind in T.KINDS:
            for mask in T.MASKS:
                inp, ref = T.reference(shape, kind, mask)
                groups = [T.system_errors(T.system_ref(*inp, dtype=torch.float32), ref)]
                if gpu:
                    groups.append(T.system_errors(T._gpu_system(*inp, "packed")[0], ref))
                row(T._id(shape), kind, mask, SYS_COLS, groups)
    emit()
    for grp in T.GROUPS:
        for i, h in enumerate(heads):
            emit("max, %-5s %-9s: " % (grp, h) + "  ".join("%s %.2e" % (c, worst[(grp, i, c)]) for c in FLOW_COLS + SYS_COLS))

    emit()
    emit("recovery, one level of stride 1, 8 evaluations, intensity features, the default mu schedule")
    gap = 0.0
    for vol in T.RECOVERY_VOLS:
        moving, fixed, star = T.recovery_fixture(vol)
        mov, fix = moving.float(), fixed.float()
        t64, h64 = T.affine_init_ref(mov, fix, levels=(1,), iters=8)
        t32, h32 = T.affine_init_ref(mov, fix, levels=(1,), iters=8, dtype=torch.float32, theta_dtype=torch.float32)
        emit("%-10s float64 loop: max |theta - theta*| %.3e, L %.3e -> %.3e" % (T._id(vol), float((t64 - star).abs().max()),
                                                                                float(h64[0, 0, 0]), float(h64[-1, 0, 1])))
        g = float((t32.double() - t64).abs().max())
        gap = max(gap, g)
        emit("%-10s fp32 CPU loop: max |theta - theta(float64 loop)| %.3e, L -> %.3e" % (T._id(vol), g, float(h32[-1, 0, 1])))
        if gpu:
            from dfmir_amd import infer
            out = infer.affine_init(mov.to(T.DEV), fix.to(T.DEV), features='intensity', levels=(1,), iters=8)
            emit("%-10s affine_init:   max |theta - theta(float64 loop)| %.3e, L -> %.3e"
                 % (T._id(vol), float((out['theta'].cpu().double() - t64).abs().max()), float(out['history'][-1, 0, 1])))
    emit("max fp32 gap of the loop: %.3e" % gap)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
