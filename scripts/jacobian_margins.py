"""The yardstick of tests/test_jacobian.py: how far the Jacobian-determinant definition (penalty and gradient, map,
statistics) evaluated by torch in fp32 on the CPU lies from the float64 restatement, per case of the test's set and per
input family, and -- when a HIP device is present -- how far the kernels lie.  profiles/jacobian_margins.txt records the
output; the test's bounds are 4x the maxima of the fp32 columns, per family.  A row holds the maxima over the test's
(power, eps) rows with a non-zero loss: the loss (relative), the gradient in relative 2-norm and as max-abs over max; then
absolute errors: the map, min d, max d, mean d, mean l, std l (l with the family's log offset).  The two masked rows (the
fields of test_jacobian_loss_mask_and_loss_mult) are listed beside them and do not enter the maxima.

    python scripts/jacobian_margins.py [--out profiles/jacobian_margins.txt]        # CPU columns only without a device
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_jacobian as T  # noqa: E402
from tests.golden import common as C  # noqa: E402

NAMES = ("loss", "grad-l2", "grad-max", "map", "min", "max", "mean", "mean-l", "std-l")


def penalty_errors(u, border, combos, gpu):
    """The maxima over `combos` of the three penalty errors, fp32 CPU and (gpu) kernels."""
    worst = [0.0] * (6 if gpu else 3)
    for power, eps in combos:
        l64, g64 = T.penalty_loss_ref(u, eps, power, border)
        if l64 == 0.0:
            continue
        r = list(T.rel_errors(*T.penalty_loss_ref(u, eps, power, border, dtype=torch.float32), l64, g64))
        if gpu:
            r += list(T.rel_errors(*T._gpu(u, eps, power, border), l64, g64))
        worst = [max(w, v) for w, v in zip(worst, r)]
    return worst[:3], worst[3:]


def map_stat_errors(u, border, off, gpu):
    x = u.double()
    m64, s64 = T.detmap_ref(x, border), T.stats_ref(x, border, off)
    cpu = [float((T.detmap_ref(u, border).double() - m64).abs().max())] + list(T.stat_errors(T.stats_ref(u, border, off), s64))
    ker = []
    if gpu:
        from dfmir_amd import ops
        d = u.to(T.DEV)
        ker = [float((ops.jacobian_determinant(d, border).cpu().double() - m64).abs().max())] + \
            list(T.stat_errors(ops.jacobian_stats(d, border, off).cpu(), s64))
    return cpu, ker


def row(u, border, family, combos, gpu):
    p32, pk = penalty_errors(u, border, combos, gpu)
    s32, sk = map_stat_errors(u, border, T.LOG_OFFSET[family], gpu)
    return p32 + s32 + pk + sk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gpu = torch.cuda.is_available()
    n = 18 if gpu else 9
    L = ["%-20s %-5s | fp32 CPU: %s%s" % ("case", "fam", "  ".join("%-8s" % s for s in NAMES),
                                         " | kernels: " + "  ".join("%-8s" % s for s in NAMES) if gpu else "")]
    fmt = lambda name, fam, r: L.append("%-20s %-5s | %s" % (name, fam, "  ".join("%.2e" % v for v in r)))
    worst = {f: [0.0] * n for f in T.FAMILIES}
    for case in T.CASES:
        for fam in T.FAMILIES:
            T.input_conditions(case, fam)
            r = row(T.reference(case, fam)["u"], case[1], fam, T.COMBOS, gpu)
            worst[fam] = [max(w, v) for w, v in zip(worst[fam], r)]
            fmt(T._id(case), fam, r)
    for fam in T.FAMILIES:
        fmt("max", fam, worst[fam])
    for shape in T.MID:
        u = T.reference((shape, 1), "fold")["u"]
        mask = (C.rand(77, *((shape[0], 1) + shape[2:])) > 0.3).float()
        fmt("masked " + "x".join(str(v) for v in shape[2:]), "fold", row(u * mask, 1, "fold", ((2, 0.5),), gpu))
    head = ["Jacobian determinant (tests/test_jacobian.py): how far the definition evaluated by torch in fp32 on the CPU lies from",
            "the float64 restatement%s, per case of the test's set" % (", and how far the HIP kernels (dfmir_amd/csrc/jacdet.hip) lie" if gpu else ""),
            "and per input family.  Output of `python scripts/jacobian_margins.py`%s." % (" on an MI355X box" if gpu else " on a machine without a GPU (no kernel columns)"),
            "loss: relative error; grad-l2: |g - g64| / |g64| in the 2-norm; grad-max: max |g - g64| / max |g64| -- the maxima over",
            "(power, eps) = (2, 0), (2, 0.5), (1, 0) where the loss is not 0; map, min, max, mean, mean-l, std-l: absolute errors of the",
            "determinant map and of the statistics (l = log(max(d + offset, 1e-9)), offset 3 for fold and 0 for mild).  fold: three",
            "sinusoids per channel whose amplitudes add up to 3 voxels, wavelengths 12 to 24 voxels; mild: the same with 0.5.",
            "", "The test bounds every comparison with the restatement by 4x the maximum of the fp32 CPU columns over the cases, per family:"]
    for fam in T.FAMILIES:
        head.append("  %-5s %s" % (fam, "  ".join("%s 4 x %.2e" % (s, v) for s, v in zip(NAMES, worst[fam][:9]))))
    if gpu:
        head.append("The kernels' maxima over the fp32 CPU maxima:")
        for fam in T.FAMILIES:
            head.append("  %-5s %s" % (fam, "  ".join("%s %.2fx" % (s, k / c if c else float('nan'))
                                                      for s, c, k in zip(NAMES, worst[fam][:9], worst[fam][9:]))))
    text = "\n".join(head + [""] + L) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
