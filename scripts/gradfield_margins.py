"""The yardstick of tests/test_gradfield.py: how far the normalised-gradient-field definition evaluated by torch in fp32 on
the CPU lies from the float64 restatement, per case of the test's set, and -- when a HIP device is present -- how far the
kernels lie.  profiles/gradfield_margins.txt records the output; the test's bounds are 4x the maxima of the fp32 columns,
floored at 1e-6 (the field: max-abs error over max).

    python scripts/gradfield_margins.py            # CPU columns only without a device
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_gradfield as T  # noqa: E402


def main():
    gpu = torch.cuda.is_available()
    print("case                          | fp32 CPU: loss  grad-l2  grad-max  field | kernels: loss  grad-l2  grad-max  field")
    worst = [0.0] * 8
    for case in T.CASES:
        shape, eps, spacing, _ = case
        a, b, l64, da64, db64 = T.reference(case)
        l32, da32, db32 = T.gradfield_loss_ref(a, b, eps, 1.0, spacing, dtype=torch.float32)
        row = list(T.rel_errors(l32, (da32, db32), l64, (da64, db64)))
        feps = eps if eps == 'auto' else eps[0]
        f64 = T.field_ref(a.double(), feps, 1.0, spacing)
        row.append(T.field_error(T.field_ref(a.float(), feps, 1.0, spacing), f64))
        if gpu:
            from dfmir_amd import ops
            got = T._gpu_loss(a, b, eps, 1.0, spacing)
            row += list(T.rel_errors(got[0], got[1:], l64, (da64, db64)))
            row.append(T.field_error(ops.gradfield_normals(a.to(T.DEV), feps, 1.0, spacing), f64))
        worst = [max(w, v) for w, v in zip(worst, row + [0.0] * (8 - len(row)))]
        print("%-29s | %s" % (T._id(case), "  ".join("%.2e" % v for v in row)))
    print("%-29s | %s" % ("max", "  ".join("%.2e" % v for v in worst[:8 if gpu else 4])))


if __name__ == "__main__":
    main()
