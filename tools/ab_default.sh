#!/bin/bash
# tools/ab_default.sh [N] : the DEFAULT bench (the headline `value`) alternating between scratch/libkwy_old.so and
# scratch/libkwy_new.so on one machine, N (default 5) runs each: old, new, old, new, ...  -> $KWY_MEASURE_OUT/ab/ab_{old,new}_i.json
# (default: measure_out/ab/ in the repository root)
# (tools/ab_libs.sh does the same with --full for the per-kernel durations).  A gain counts when the difference of the
# means is at least three times the larger of the two builds' run-to-run ranges.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
N=${1:-5}
O=${KWY_MEASURE_OUT:-$R/measure_out}/ab
mkdir -p $O
cd $R
cp kwiiyatta_amd/libkwy.so scratch/libkwy_tree.so
for i in $(seq 1 $N); do
  for v in old new; do
    cp scratch/libkwy_$v.so kwiiyatta_amd/libkwy.so
    timeout -k 10 200 python bench.py > $O/ab_${v}_$i.json 2> $O/ab_${v}_$i.err || { tail -5 $O/ab_${v}_$i.err; cp scratch/libkwy_tree.so kwiiyatta_amd/libkwy.so; exit 1; }
  done
done
cp scratch/libkwy_tree.so kwiiyatta_amd/libkwy.so
python - "$O" "$N" <<'PY'
import json, sys
o, n = sys.argv[1], int(sys.argv[2])
res = {v: [json.loads(open(f'{o}/ab_{v}_{i}.json').read().strip().splitlines()[-1])['value'] for i in range(1, n + 1)] for v in ('old', 'new')}
mean = {v: sum(r) / len(r) for v, r in res.items()}
rng = {v: (max(r) - min(r)) / mean[v] for v, r in res.items()}
out = {'runs': res, 'mean': mean, 'range_rel': rng, 'gain_rel': mean['new'] / mean['old'] - 1.0,
       'gain_over_larger_range': (mean['new'] / mean['old'] - 1.0) / max(rng.values())}
print(json.dumps(out, indent=1))
open(f'{o}/ab_summary.json', 'w').write(json.dumps(out, indent=1) + '\n')
PY
