#!/bin/bash
# headline throughput vs streams in flight (each line one bench run, no CPU baseline); hardware queues are left to the environment
set -o pipefail
run() { timeout -k 10 200 python bench.py --streams $1 --steps ${STEPS:-12} --warmup 2 --no-cpu-baseline --no-h2d 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('streams $1:', d['value'], d['ms_per_step'])" || exit 1; }
for s in ${STREAMS:-32 40 48 64}; do run $s; done
