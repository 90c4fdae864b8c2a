#!/bin/bash
# GPU-box validation run: build check, box-tier tests, bench (default + single process),
# BASELINE configs, CPU profile of one consumer. Every step has its own time limit.
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
root=$PWD
out="${BOX_OUT:-$root/bench_out}"
mkdir -p "$out"
lscpu > "$out/lscpu.txt" 2>&1
cat /sys/fs/cgroup/cpu.max > "$out/cgroup_cpu_max.txt" 2>&1
python -c "import bench; print(bench.available_cpus())" > "$out/available_cpus.txt" 2>&1
timeout -k 10 300 python __graft_entry__.py > "$out/entry.log" 2>&1 &&
timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$out/pytest_gpu.log" 2>&1 &&
timeout -k 10 300 python bench.py --full > "$out/bench.json" 2> "$out/bench.err" &&
timeout -k 10 300 python bench.py --full --procs-per-rank 1 > "$out/bench_1proc.json" 2> "$out/bench_1proc.err" &&
timeout -k 10 600 python -m beholder_amd bench all --out "$out/baseline_configs.json" > "$out/baseline.log" 2>&1 &&
timeout -k 10 300 python scripts/profile_consumer.py > "$out/cprofile_consumer.txt" 2>&1
# rocprofv3 kernel trace of the flagship bench: documents that the path dispatches no GPU kernels
if [ $? -eq 0 ] && [ "${SKIP_ROCPROF:-0}" != "1" ]; then
  ( cd /tmp && export TMPDIR=/tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats \
      -d "$out/rocprof" -o bench -- python3 "$root/bench.py" \
      --steps 3 --warmup 1 --procs-per-rank 1 > "$out/rocprof_bench.log" 2>&1 )
  echo "rocprof rc=$?" >> "$out/rocprof_bench.log"
  (find "$out/rocprof" -type f 2>/dev/null || echo "no rocprof output files (no kernel dispatches)") \
    > "$out/rocprof_files.txt"
fi
true
