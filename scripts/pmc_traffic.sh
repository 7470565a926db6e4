#!/bin/bash
# HBM traffic of the bench's kernels from the PMC counters, collected as MI355X_MICROARCH.md
# prescribes: FETCH_SIZE and WRITE_SIZE in SEPARATE rocprofv3 passes, kernel-trace only.
# usage (on the GPU box): bash scripts/pmc_traffic.sh <output dir, relative to the repository root> [bench args...]
# then: python scripts/pmc_traffic.py <output dir> out.json
# Each pass runs under a time limit; the first pass that fails, faults or times out ends the script.
OUT=$1; shift
export TMPDIR=/tmp
cd "$(dirname "$0")/.." || exit 1
mkdir -p "$OUT"
for c in FETCH_SIZE WRITE_SIZE; do
  log=$OUT/$c.log
  timeout -k 10 600 rocprofv3 --pmc $c --kernel-trace --output-format csv -d "$OUT/$c" -- python bench.py --steps 1 --warmup 1 --no-cpu-baseline "$@" > "$log" 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "pass $c failed (exit $rc)"; tail -3 "$log"; exit 1; fi
  if grep -q "fault" "$log"; then echo FAULT; exit 1; fi
  echo "pass $c done"
done
