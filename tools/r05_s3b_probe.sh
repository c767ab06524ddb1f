#!/bin/bash
# round 5: the strong-scaling budget at S3b (bowl3D h = 0.0125, 8.97 M unknowns): one GPU's serial cycle and rank 4 of 8's distributed cycle, one box
cd "${GRAFT_REPO_ROOT:-.}" || exit 1
O=${BENCH_OUT:-bench_out}; mkdir -p "$O"
timeout -k 10 500 python3 bench.py --full --workload bowl3D_h0.0125 --steps 1 --warmup 1 --no-multigrid --no-cpu-baseline > "$O/r05_s3b_serial.json" 2> "$O/r05_s3b_serial.err" || { echo "serial bench failed"; tail -5 "$O/r05_s3b_serial.err"; exit 1; }
python3 tools/bench_ab_summary.py "$O/r05_s3b_serial.json"
NPG_COMM_SELFTEST=1 NPG_COMM_TRANSPORT=peer timeout -k 10 500 python3 tools/rank_cycle_probe.py bowl3D_h0.0125 8 4 ${S3B_ITS:-600} > "$O/r05_s3b_rank.txt" 2> "$O/r05_s3b_rank.err" || { echo "rank probe failed"; tail -5 "$O/r05_s3b_rank.err"; exit 1; }
cat "$O/r05_s3b_rank.txt"
