#!/bin/bash
# lanes inside one handle at the default workload: is the overlap of two half-batches worth anything with this round's kernels?
#   bash tools/experiments/handle_lanes.sh OUTDIR
set -e
OUT=${1:?usage: handle_lanes.sh OUTDIR}
mkdir -p $OUT
for l in 1 2; do
  for p in 16 32; do
    python bench.py --full --steps 30 --warmup 5 --cpu-seconds 0 --call-site 0 --pairs $p --lanes $l > $OUT/lanes_l${l}_p${p}.json 2> $OUT/lanes_l${l}_p${p}.err
    python - <<PY
import json
d=json.loads(open("$OUT/lanes_l${l}_p${p}.json").read().strip().splitlines()[-1])
print("lanes $l pairs $p:", d["value"], d["ms_per_step"], d.get("parity_checksum_ok"))
PY
  done
done
