"""The yardstick of tests/test_landmarks.py: how far the landmark definition evaluated by torch in fp32 on the CPU lies from
the float64 restatement, per case and variant of the test's set, and -- when a HIP device is present -- how far the kernels
lie.  profiles/landmark_margins.txt records the output; the test's bounds are 4x the maxima of the fp32 CPU columns.  Nothing
is excluded: every landmark and every voxel of dflow takes part (the NaN patterns must agree exactly).

    python scripts/landmark_margins.py            # CPU columns only without a device
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_landmarks as T  # noqa: E402

COLS = "loss  d-max  mapped-max  dflow-l2  dflow-max"


def row(case, variant, gpu):
    flow, q, p, w, h, ref = T.reference(case, variant)
    r = list(T.errors(T.lm_ref(flow, q, p, w, h, variant[0], dtype=torch.float32), ref))
    if gpu:
        r += list(T.errors(T._gpu(flow, q, p, w, h, variant[0]), ref))
    return r


def main():
    gpu = torch.cuda.is_available()
    n = 10 if gpu else 5
    print("loss: relative; d, mapped: max-abs (voxels x spacing, voxels); dflow: relative 2-norm, max-abs over max")
    print("case                  variant        | fp32 CPU: %s%s" % (COLS, " | kernels: " + COLS if gpu else ""))
    fmt = lambda name, var, r: print("%-21s %-14s | %s" % (name, var, "  ".join("%.2e" % x for x in r)))
    worst = [0.0] * n
    for case in T.CASES:
        for variant in T.VARIANTS:
            if case[1] == T.MAX_K and variant != T.VARIANTS[1]:          # the maximum K runs once in the test
                continue
            r = row(case, variant, gpu)
            worst = [max(a, b) for a, b in zip(worst, r)]
            fmt(T._id(case), T._vid(variant), r)
    fmt("max", "", worst)
    if gpu:
        print("kernels / fp32 CPU     " + " " * 14 + " | " + "  ".join("%.2f" % (worst[5 + i] / worst[i]) for i in range(5)))


if __name__ == "__main__":
    main()
