"""The yardstick of tests/test_invcons.py: how far the inverse-consistency definition evaluated by torch in fp32 on the CPU
lies from the float64 restatement, per case of the test's set, per input family and for the one-way and the symmetric form,
and -- when a HIP device is present -- how far the kernels lie.  profiles/invcons_margins.txt records the output; the test's
bounds are 4x the maxima of the fp32 columns, per family.  The du columns leave out what the test leaves out (smooth family:
voxels with a sample coordinate within 1e-4 of an integer).

    python scripts/invcons_margins.py            # CPU columns only without a device
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_invcons as T  # noqa: E402

COLS = "loss  du-l2  du-max  dv-l2  dv-max"


def row(shape, fam, symmetric, gpu):
    u, v, ref, keeps = T.reference(shape, fam, symmetric)
    r = list(T.all_errors(T.ic_loss_ref(u, v, symmetric, dtype=torch.float32), ref, keeps))
    if gpu:
        r += list(T.all_errors(T._gpu(u, v, symmetric), ref, keeps))
    return r


def main():
    gpu = torch.cuda.is_available()
    n = 10 if gpu else 5
    print("case                  form      family  | fp32 CPU: %s%s" % (COLS, " | kernels: " + COLS if gpu else ""))
    fmt = lambda name, form, fam, r: print("%-21s %-9s %-7s | %s" % (name, form, fam, "  ".join("%.2e" % x for x in r)))
    worst = {f: [0.0] * n for f in T.FAMILIES}
    for shape in T.SHAPES:
        for symmetric in (False, True):
            for fam in T.FAMILIES:
                r = row(shape, fam, symmetric, gpu)
                worst[fam] = [max(w, x) for w, x in zip(worst[fam], r)]
                fmt(T._id(shape), "symmetric" if symmetric else "one-way", fam, r)
    for fam in T.FAMILIES:
        fmt("max", "", fam, worst[fam])


if __name__ == "__main__":
    main()
