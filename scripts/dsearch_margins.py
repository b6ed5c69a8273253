"""The yardstick of tests/test_dsearch.py: how far the definitions of ops.pool_features, ops.ssd_cost_volume and
ops.box_smooth_flow evaluated by torch in fp32 on the CPU lie from the float64 restatement, per case of the test's set, and --
when a HIP device is present -- how far the kernels lie.  profiles/dsearch_margins.txt records the output; the test's bounds are
4x the row "max" of the fp32 CPU columns, per quantity.  Per quantity: max-abs over max, relative 2-norm.  Also, per case, the
argmin on the kernel's own cost volume: the worst J64[idx] - min J64 over the voxels and coefficients beside the test's tau,
and the share of picks that differ from the float64 argmin (near-ties: not an error, and not asserted).

    python scripts/dsearch_margins.py            # CPU columns only without a device
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_dsearch as T  # noqa: E402
from tests.golden import common as C  # noqa: E402

F32 = torch.float32


def fmt(name, r):
    print("%-24s | %s" % (name, "  ".join("%.2e" % x for x in r)))


def main():
    gpu = torch.cuda.is_available()
    cols = "pool-max  pool-l2  cost-max  cost-l2  smooth-max  smooth-l2"
    print("%-24s | fp32 CPU: %s%s" % ("case (B,C,*vol)-g-r", cols, " | kernels: " + cols if gpu else ""))
    if gpu:
        from dfmir_amd import ops
    rows, argmin_lines = [], []
    for case in T.CASES:
        shape, g, r = case
        ref = T.reference(case)
        mov_p, fix_p = ref["P"]
        d = T.integer_field(case)
        s64 = T.smooth_ref(d.double())
        pool = [T.errs(T.pool_ref(ref[n], g), p64) for n, p64 in zip(("mov", "fix"), ref["pooled64"])]
        row = [max(e[0] for e in pool), max(e[1] for e in pool)]
        row += list(T.errs(T.cost_ref(fix_p, mov_p, r), ref["cost64"]))
        row += list(T.errs(T.smooth_ref(d), s64))
        if gpu:
            pool = [T.errs(ops.pool_features(ref[n].to(T.DEV), g), p64) for n, p64 in zip(("mov", "fix"), ref["pooled64"])]
            row += [max(e[0] for e in pool), max(e[1] for e in pool)]
            cost = ops.ssd_cost_volume(fix_p.to(T.DEV), mov_p.to(T.DEV), r)
            row += list(T.errs(cost, ref["cost64"]))
            row += list(T.errs(ops.box_smooth_flow(d.to(T.DEV)), s64))
            nd = mov_p.dim() - 2
            soft = (C.rand(2300 + T.CASES.index(case), mov_p.shape[0], nd, *mov_p.shape[2:]) * 2 - 1) * r
            for coeff in (0.0, 0.003, 1.0):
                idx = ops.cost_argmin(cost, r, soft.to(T.DEV), coeff)[0].cpu().long()
                J = T.coupled_ref(ref["cost64"], r, soft, coeff)
                gap = float((J.gather(1, idx[:, None])[:, 0] - J.min(1).values).max())
                tau = 2.0 * (T.BOUND["cost"][0] * float(ref["cost64"].abs().max()) + coeff * T.EPS32 * (2 * r) ** 2 * nd)
                share = float((idx != T.argmin_ref(ref["cost64"], r, soft, coeff)[0]).float().mean())
                argmin_lines.append("%-24s coeff %-5g | worst gap %.2e  tau %.2e  picks that differ from the float64 argmin %.4f"
                                    % (T._id(case), coeff, gap, tau, share))
        rows.append(row)
        fmt(T._id(case), row)
    fmt("max", [max(col) for col in zip(*rows)])
    if argmin_lines:
        print("\ncost_argmin on the kernel's cost volume, soft = noise in [-r, r]")
        print("\n".join(argmin_lines))


if __name__ == "__main__":
    main()
