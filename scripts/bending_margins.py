"""The yardstick of tests/test_bending.py: how far the bending-energy definition evaluated by torch in fp32 on the CPU lies
from the float64 restatement, per case of the test's set and per input family, and -- when a HIP device is present -- how
far the kernels lie.  profiles/bending_margins.txt records the output; the test's bounds are 4x the maxima of the fp32
columns, per family.  The two masked rows (the field of test_bending_loss_mask_and_loss_mult) are listed beside them and do
not enter the maxima.

    python scripts/bending_margins.py            # CPU columns only without a device
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_bending as T  # noqa: E402
from tests.golden import common as C  # noqa: E402


def row(u, sp, gpu):
    l64, g64 = T.bending_loss_ref(u, sp)
    l32, g32 = T.bending_loss_ref(u, sp, dtype=torch.float32)
    r = list(T.rel_errors(l32, g32, l64, g64))
    if gpu:
        r += list(T.rel_errors(*T._gpu(u, sp), l64, g64))
    return r


def main():
    gpu = torch.cuda.is_available()
    n = 6 if gpu else 3
    print("case                      family | fp32 CPU: loss  grad-l2  grad-max%s" % (" | kernels: loss  grad-l2  grad-max" if gpu else ""))
    fmt = lambda name, fam, r: print("%-25s %-6s | %s" % (name, fam, "  ".join("%.2e" % v for v in r)))
    worst = {f: [0.0] * n for f in T.FAMILIES}
    for case in T.CASES:
        shape, spaced = case
        for fam in T.FAMILIES:
            r = row(T.reference(case, fam)[0], T._spacing(shape, spaced), gpu)
            worst[fam] = [max(w, v) for w, v in zip(worst[fam], r)]
            fmt(T._id(case), fam, r)
    for fam in T.FAMILIES:
        fmt("max", fam, worst[fam])
    for shape in ((2, 3, 13, 17, 19), (1, 2, 37, 41)):
        u = T.reference((shape, True), "noise")[0]
        mask = (C.rand(77, *((shape[0], 1) + shape[2:])) > 0.3).float()
        fmt("masked " + "x".join(str(v) for v in shape), "noise", row(u * mask, T._spacing(shape, True), gpu))


if __name__ == "__main__":
    main()
