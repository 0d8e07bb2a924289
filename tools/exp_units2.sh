#!/bin/bash
# More of tools/exp_units.sh: rounds of long units per wave.
cd "${GRAFT_REPO_ROOT:-$(pwd)}"
trap 'python3 ohpipeline_amd/build.py --force > /dev/null 2>&1' EXIT     # an interrupted experiment must not leave a diagnostic library behind
OHGPU_EXTRA_FLAGS="-DOHGPU_DIAG -DOHGPU_DIAG_ONE_KERNEL" python3 ohpipeline_amd/build.py --force > /dev/null 2>&1 || { echo "build failed"; exit 1; }
for envs in "X=1" "OHGPU_DIAG_LONG_ROUNDS=1" "OHGPU_DIAG_LONG_ROUNDS=3" "OHGPU_DIAG_LONG_ROUNDS=1 OHGPU_DIAG_TAIL_ROUNDS=1.0" "OHGPU_DIAG_TAIL_ROUNDS=1.0" "OHGPU_DIAG_TAIL_ROUNDS=2.0" "OHGPU_DIAG_KB_MAX=1" "X=2"; do
  echo -n "$envs: "
  env $envs timeout -k 10 120 python3 bench.py --full --steps 300 --warmup 20 --no-cpu | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['roofline']['kernel_avg_ms'], d['roofline']['frac'], d['plan_ms'])"
done
python3 ohpipeline_amd/build.py --force > /dev/null 2>&1
