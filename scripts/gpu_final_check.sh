#!/bin/bash
# round-end checks on one box: the GPU suite twice (tolerance tests against split-K atomics: flakiness shows here), smoke, and
# the default bench command with its wall clock, then the --full line.   scripts/gpu_final_check.sh <output directory>
# Every GPU step runs under its own time limit; the script stops at the first step that fails, faults or times out.
set -e -o pipefail
O=${1:?usage: scripts/gpu_final_check.sh <output directory>}
mkdir -p $O
for i in 1 2; do
  timeout -k 10 1500 python -m pytest tests -m gpu -x -q > $O/pytest_$i.txt 2>&1 || { tail -5 $O/pytest_$i.txt; exit 1; }
  tail -1 $O/pytest_$i.txt
done
timeout -k 10 600 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.txt 2>&1 || { tail -5 $O/smoke.txt; exit 1; }
tail -1 $O/smoke.txt
T0=$SECONDS
timeout -k 10 600 python bench.py > $O/bench_default.json 2> $O/bench_default.err
echo "default bench: $((SECONDS - T0)) s wall"
timeout -k 10 900 python bench.py --full > $O/bench_full.json 2> $O/bench_full.err
python - $O/bench_full.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['roofline']['issued_frac'], d['roofline']['single_stream'], d['also_3d']['ms_per_step'], d['also_3d_128']['ms_per_step'])
PY
