"""The yardstick of tests/test_demons.py: how far the demons definitions evaluated by torch in fp32 on the CPU lie from the
float64 restatement, per case of the test's set -- ops.gaussian_smooth (relative 2-norm and max-abs over max, per shape and
sigma), ops.demons_force (d in relative 2-norm and max-abs over max, L and L_b relative, per shape, flow kind and mask) -- and,
when a HIP device is present, how far the kernels lie; then infer.demons_flow on the two fixtures and its variants: the fp32 CPU
restatement of the whole loop against the float64 loop (max |flow gap| in voxels, max relative gap of the history), and the
driver itself against the float64 loop.  The test's bounds are 4x the maxima of the fp32 columns -- over the small shapes and
over the large ones separately -- and 4x the fp32 gap of each loop.  The fp32 figures depend on the host's thread count;
profiles/ keeps a run on a host with the device (demons_margins.txt) and one on a host without (demons_margins_cpu.txt), and the
test quotes the smaller figure per quantity.

    python scripts/demons_margins.py [out.txt]       # default profiles/demons_margins.txt; CPU columns only without a device
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import test_demons as T  # noqa: E402

GAUSS_COLS = ("l2", "max")
FORCE_COLS = ("d_l2", "d_max", "L", "Lb")
LOOP_COLS = ("flow", "history")


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "demons_margins.txt")
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    gpu = torch.cuda.is_available()
    heads = ["fp32 CPU"] + (["kernels"] if gpu else [])
    worst = {}

    def row(what, grp, label, cols, groups):
        emit("%-34s | %s" % (label, " | ".join("  ".join("%.2e" % g[c] for c in cols) for g in groups)))
        for i, g in enumerate(groups):
            for c in cols:
                worst[(what, grp, i, c)] = max(worst.get((what, grp, i, c), 0.0), g[c])

    emit("gaussian_smooth: " + "  ".join(GAUSS_COLS) + "      (" + " | ".join(heads) + ")")
    extra = [((2, 3, 6, 10, 12), (1.2, 0.0, 0.0)), ((2, 3, 6, 10, 12), 1.2)]
    for shape, sigma in T.GAUSS_CASES + extra:
        x = T.gauss_input(shape)
        ref = T.gauss_ref(x, sigma)
        groups = [T.field_errors(T.gauss_ref(x, sigma, dtype=torch.float32), ref)]
        if gpu:
            groups.append(T.field_errors(T._gpu_gauss(x, sigma), ref))
        sg = sigma if isinstance(sigma, tuple) else (round(sigma, 3),)
        row("gauss", T.group_of(shape), "%-16s sigma %s" % (T._id(shape), "/".join("%g" % s for s in sg)), GAUSS_COLS, groups)
    emit()
    emit("demons_force (max_step %g): " % T.MAX_STEP + "  ".join(FORCE_COLS) + "      (" + " | ".join(heads) + ")")
    for shape in T.FORCE_SHAPES:
        for kind in T.KINDS:
            for mask in T.MASKS:
                inp, ref = T.force_reference(shape, kind, mask)
                groups = [T.force_errors(T.demons_force_ref(*inp, dtype=torch.float32), ref)]
                if gpu:
                    groups.append(T.force_errors(T._gpu_force(*inp, "packed")[0], ref))
                row("force", "small", "%-14s %-8s %-8s" % (T._id(shape), kind, mask), FORCE_COLS, groups)
    emit()
    for what, cols in (("gauss", GAUSS_COLS), ("force", FORCE_COLS)):
        for grp in ("small", "large"):
            for i, h in enumerate(heads):
                if (what, grp, i, cols[0]) in worst:
                    emit("max, %-5s %-5s %-9s: " % (what, grp, h) + "  ".join("%s %.2e" % (c, worst[(what, grp, i, c)]) for c in cols))
    emit()
    emit("demons_flow, levels (2, 1), both sigmas 1, max_step 2, intensity features: " + "  ".join(LOOP_COLS)
         + "      (fp32 CPU loop" + (" | infer.demons_flow" if gpu else "") + ", both against the float64 loop)")
    for name, variant in (("2d", "compose"), ("3d", "compose"), ("2d", "add"), ("2d", "diffeomorphic")):
        ref = T.loop_reference(name, variant)
        groups = [T.loop_errors(T.loop_reference(name, variant, torch.float32), ref)]
        if gpu:
            groups.append(T.loop_errors(T._gpu_loop(name, variant), ref))
        emit("%-3s %-14s energy %.3e -> %.3e (ratio %.4f) | %s" % (
            name, variant, float(ref['energy0']), float(ref['energy']), float(ref['energy'] / ref['energy0']),
            " | ".join("  ".join("%.2e" % g[c] for c in LOOP_COLS) for g in groups)))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
