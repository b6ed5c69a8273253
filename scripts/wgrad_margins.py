#!/usr/bin/env python
"""CPU only: the fp32 yardsticks of tests/test_gpu_wgrad_fp64.py.  For every case of tests/wgrad_cases.py (the branch cases, the
edge runs on the fp32 hosts, the 7x7 stem, the bias cases) the error of the fp32 restatement of tests/ref64.py against float64,
the larger of its two evaluation orders ('matmul', 'chunk64'), as largest per-output-channel relative 2-norm and as max-abs
over max; then the maximum per family -- the constants FP32_YARD of the test module (its bounds are FACTOR = 4 x these).
Beside them, where given, the kernels' measured errors per accumulation mode from a GPU run of the test module
(--measured FILE: the lines the module prints with DFMIR_WGRAD_PRINT=1 under pytest -s); no bound is derived from that column.
--before FILE: such a log of the deterministic tests on a library with the earlier scale rule (the fp32 product
count * max(max|x|, 1) * max|dy|); its rows beyond their bound are listed at the end.

    python scripts/wgrad_margins.py [--measured gpu_log.txt] [--before gpu_log_before.txt] > profiles/wgrad_margins.txt
"""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import wgrad_cases as WC  # noqa: E402


def family(c):
    return "%dd" % c["nd"]


def measured_table(path):
    """{(case key, what, mode): (l2, max)} from lines 'WGRAD <mode> <key> <what> l2=<e> max=<e> ...'."""
    out = {}
    if not path:
        return out
    pat = re.compile(r"WGRAD (\S+) (\S+) (\S+) l2=(\S+) max=(\S+)")
    for line in open(path):
        m = pat.search(line)
        if m:
            k = (m.group(2), m.group(3), m.group(1))
            v = (float(m.group(4)), float(m.group(5)))
            out[k] = tuple(max(a, b) for a, b in zip(out.get(k, (0.0, 0.0)), v))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measured", default=None)
    ap.add_argument("--before", default=None)
    a = ap.parse_args()
    meas = measured_table(a.measured)
    fam = {}

    def row(key, what, f, e, kind):
        cols = ""
        for mode in ("atomic", "deterministic"):
            m = meas.get((key, what, mode))
            cols += "  %9s %9s" % (("%.2e" % m[0], "%.2e" % m[1]) if m else ("-", "-"))
        print("%-34s %-3s %-5s %-4s  %9.2e %9.2e%s" % (key, what, kind, f, e[0], e[1], cols))
        if kind == "fp32":
            fam[f, what] = tuple(max(p, q) for p, q in zip(fam.get((f, what), (0.0, 0.0)), e))

    print("# fp32 CPU restatement (tests/ref64.py conv_weight_grad / conv_bias_grad, the larger of the orders %s) against float64,"
          % (WC.ORDERS,))
    print("# and the HIP kernels' measured errors per accumulation mode (MI355X; '-' = not measured).  l2 = largest per-output-channel")
    print("# relative 2-norm error, max = max-abs error over max |reference|.  Bounds of the fp32 kernels: 4 x the family maxima")
    print("# below (FP32_YARD in tests/test_gpu_wgrad_fp64.py); split kernels: the project's figures (see that module).")
    print("%-34s %-3s %-5s %-4s  %9s %9s  %9s %9s  %9s %9s" % ("case", "", "kind", "fam", "cpu l2", "cpu max", "atomic l2", "atomic mx",
                                                               "determ l2", "determ mx"))
    runs = [(c, None) for c in WC.CASES] + [(WC.STEM7, None)] + [(WC.BY_ID[h], e) for h, e in WC.EDGE_RUNS]
    for c, edge in runs:
        if edge in ("zero_input", "zero_dy"):
            continue                                             # exact zeros: no relative error to speak of
        x, dy = WC.inputs(c, edge)
        ew, eb, _ = WC.yardstick(c, x, dy)
        key = c["id"] + ("+" + edge if edge else "")
        row(key, "dW", family(c), ew, c["kind"])
        row(key, "db", "bias", eb, c["kind"])
    for bid, N, Cc, S in WC.BIAS_CASES:
        for gs in WC.BIAS_SCALES:
            dy = WC.bias_input(N, Cc, S, gs)
            ref = WC.R.conv_bias_grad(dy)
            e = (0.0, 0.0)
            for o in WC.ORDERS:
                e = tuple(max(p, q) for p, q in zip(e, WC.rel_errors(WC.R.conv_bias_grad(dy, WC.F32, o).view(-1, 1), ref.view(-1, 1))))
            row("%s@%g" % (bid, gs), "db", "bias", e, "fp32")
    print("#")
    print("# family maxima over the fp32-kernel rows (-> FP32_YARD):")
    for (f, what), e in sorted(fam.items()):
        print("# max %-4s %-3s  %9.2e %9.2e" % (f, what, e[0], e[1]))
    if a.before:
        before_section(a.before, meas)


def before_section(path, after):
    pat = re.compile(r"WGRAD deterministic (\S+) (\S+) l2=(\S+) max=(\S+) bounds (\S+) (\S+)")
    seen = {}
    for line in open(path):
        m = pat.search(line)
        if m:
            seen[m.group(1), m.group(2)] = tuple(None if g == "None" else float(g) for g in m.groups()[2:])
    print("#")
    print("# before: deterministic mode on the library with the earlier scale rule, rows beyond their bound (1.00e+00 = every")
    print("# element zero or lost), and the same rows with the rule of include/dfmir_hip.h")
    print("# %-32s %-3s  %9s %9s  %9s %9s  %9s %9s" % ("case", "", "before l2", "before mx", "after l2", "after max", "bound l2", "bound max"))
    for (key, what), (l2, mx, b0, b1) in sorted(seen.items()):
        if (b0 is not None and l2 > b0) or mx > b1:
            a_ = after.get((key, what, "deterministic"))
            print("# %-32s %-3s  %9.2e %9.2e  %9s %9s  %9s %9.2e" % (key, what, l2, mx, "%.2e" % a_[0] if a_ else "-",
                                                                  "%.2e" % a_[1] if a_ else "-", "-" if b0 is None else "%.2e" % b0, b1))


if __name__ == "__main__":
    main()
