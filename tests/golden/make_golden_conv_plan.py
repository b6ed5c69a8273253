"""Generator of tests/golden/conv_plan.json -- the table tests/test_conv_plan.py holds ops.conv_raw / ops.conv_wgrad_raw to.
The case list, the stand-in library and the recorder are the test file's own; this script only runs them and writes the
distinct rows, one per line, and the index of every case's row in the order of the case list.

    python tests/golden/make_golden_conv_plan.py --tree <checkout>     record from <checkout>/dfmir_amd/ops.py; the file
                                                                        names that checkout's HEAD (which must be clean)
    python tests/golden/make_golden_conv_plan.py                        re-record from this tree under the commit the file
                                                                        already names: it must come out byte-identical
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=None)
    args = ap.parse_args()
    out = os.path.join(HERE, "conv_plan.json")
    if args.tree:
        tree = os.path.abspath(args.tree)
        if subprocess.check_output(["git", "-C", tree, "status", "--porcelain", "--", "dfmir_amd"]).strip():
            raise SystemExit("%s: dfmir_amd differs from its HEAD" % tree)
        commit = subprocess.check_output(["git", "-C", tree, "rev-parse", "HEAD"]).decode().strip()
        sys.path.insert(0, tree)
        import dfmir_amd.ops                                  # noqa: F401  (that tree's; the test file finds it loaded)
        sys.path.remove(tree)
    else:
        with open(out) as f:
            commit = json.load(f)["recorded_from"]
    sys.path.insert(0, REPO)
    from tests import test_conv_plan as T
    print("recording from %s" % os.path.dirname(T.ops.__file__))
    cases = T.fwd_cases() + T.wgrad_cases()
    records, rows = [], []
    for c in cases:
        r = T.dumps(T.record(c))
        if r not in records:
            records.append(r)
        rows.append(records.index(r))
    idx = [",".join(str(i) for i in rows[k:k + 40]) for k in range(0, len(rows), 40)]
    with open(out, "w") as f:
        f.write('{"recorded_from":"%s",\n"cases":"%s",\n"records":[\n%s\n],\n"rows":[\n%s\n]}\n'
                % (commit, T.ids_digest(cases), ",\n".join(records), ",\n".join(idx)))
    print("%d forward + %d weight-gradient cases, %d distinct rows -> %s (%d bytes)"
          % (len(T.fwd_cases()), len(T.wgrad_cases()), len(records), out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
