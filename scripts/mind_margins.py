"""The yardstick of tests/test_mind.py: how far the MIND-SSC definition evaluated by torch in fp32 on the CPU lies from the
float64 restatement, per case of the test's shape set, and -- when a HIP device is present -- how far the kernels lie.
profiles/mind_margins.txt records the output; the test's bounds are 4x the maxima of the fp32 columns
(the descriptor: max-abs error over max).

    python scripts/mind_margins.py            # CPU columns only without a device
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_mind as T  # noqa: E402


def main():
    gpu = torch.cuda.is_available()
    print("case                      | fp32 CPU: loss  grad-l2  grad-max  descriptor | kernels: loss  grad-l2  grad-max  descriptor")
    worst = [0.0] * 8
    cases = [(T._id(c), c, None) for c in T.CASES] + [("clamped", None, T.clamped_pair())]
    for name, case, pair in cases:
        if case is not None:
            a, b, l64, da64, db64, _ = T.reference(case)
            r, d = case[1:]
        else:
            a, b = pair
            r = d = 2
            l64, da64, db64 = T.mind_loss_ref(a, b)
        l32, da32, db32 = T.mind_loss_ref(a, b, r, d, dtype=torch.float32)
        row = list(T.rel_errors(l32, (da32, db32), l64, (da64, db64)))
        M64 = T.mind_ref(a.double(), r, d)
        row.append(float((T.mind_ref(a.float(), r, d).double() - M64).abs().max() / M64.abs().max()))
        if gpu:
            from dfmir_amd import ops
            row += list(T.rel_errors(*(lambda g: (g[0], g[1:]))(T._gpu_loss(a, b, r, d)), l64, (da64, db64)))
            M = ops.mind_descriptor(a.to(T.DEV), r, d).cpu().double()
            row.append(float((M - M64).abs().max() / M64.abs().max()))
        worst = [max(w, v) for w, v in zip(worst, row + [0.0] * (8 - len(row)))]
        print("%-25s | %s" % (name, "  ".join("%.2e" % v for v in row)))
    print("%-25s | %s" % ("max", "  ".join("%.2e" % v for v in worst[:8 if gpu else 4])))


if __name__ == "__main__":
    main()
