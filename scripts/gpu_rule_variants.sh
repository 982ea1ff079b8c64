#!/bin/bash
# Runs on the GPU box: the bench line of one config under argmin PRESS and under the Wilcoxon rule, alternating, REPS times
#   gpurun -- 'bash scripts/gpu_rule_variants.sh 3 2'
set -u
export TMPDIR=/tmp ABC_DIAG=1
CFG="$1"; REPS="${2:-2}"
mkdir -p gpurun_out
run() {   # label, rule, env assignments...
  local label="$1" rule="$2"; shift 2
  env "$@" python3 bench.py --full --config $CFG --rule $rule --steps 40 --warmup 5 --no-cpu-baseline --no-extra 2>/dev/null | tail -1 | python3 -c "
import json, sys; d=json.loads(sys.stdin.read()); print('%-34s step %.4f ms  streaming %.4f ms' % ('$label', d['ms_per_step'], d['roofline_streaming']['ms']))"
}
for r in $(seq 1 $REPS); do
  run "press" press A=1
  run "wilcoxon" wilcoxon A=1
done
