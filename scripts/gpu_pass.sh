#!/bin/bash
# The GPU pass: STEPS="..." selects steps, run in the order of this file, each
# under its own time limit.  A crash, abort or timeout ends the script (test
# failures, rc 1, do not), and so does a GPU fault text in the step's log,
# whatever the step's status: nothing more runs on a card that has faulted.
#   pytest     the GPU suite (PYTEST_ARGS, default: without the large tiles)
#   smoke      __graft_entry__.py smoke
#   bench      python bench.py --full
#   torchrun1  the driver's torchrun N=1 path (RCCL process group of one rank)
#   gloo2      2-rank gloo rehearsal of the torchrun bench
#   lines      the BASELINE config lines (C2, C3, C4, C5, MCMC, MALA, Aggregate)
#   host       host-side issue cost of a step (scripts/host_overhead.py)
#   probe      scripts/probe/issue_probe (built beforehand; compiled here if missing)
#   law        log Z and ESS by sample size (scripts/c2_law.py, LAW_RUNS)
#   paired     every oracle run of the C2 target replayed (tests/test_gpu_paired.py)
#   profile    rocprofv3 kernel trace + PMC passes of C2 (scripts/profile.sh),
#              summarised into $O/$PMC_SUMMARY (scripts/pmc_summary.py)
#   trace      the bench line's own command under a kernel trace
#   c4pmc c5pmc  the PMC passes of --workload c4 / c5 ($PMC_SUMMARY_C4 / _C5)
#   postbench  copies the PMC summaries to profiles/, then python bench.py --full
#   large      the global-memory (large-tile) tests, last
# OUT_DIR is where the logs and profiles go (default out/).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
O=${OUT_DIR:-out}
mkdir -p $O
STEPS=${STEPS:-"pytest smoke bench torchrun1 host profile large"}
# the names bench.py reads under profiles/ (PMC_FILES)
PMC_SUMMARY=${PMC_SUMMARY:-pmc_mh_r06.json}
PMC_SUMMARY_C4=${PMC_SUMMARY_C4:-pmc_mh_c4_r06.json}
PMC_SUMMARY_C5=${PMC_SUMMARY_C5:-pmc_mh_c5_r06.json}
SQ="SQ_INSTS_VALU SQ_INSTS_VALU_FLOPS_FP32 SQ_INSTS_VALU_FLOPS_FP32_TRANS SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES SQ_INSTS_SMEM"
SQ2="SQ_LDS_BANK_CONFLICT SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU"
SQ3="SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SCRATCH SQ_WAVES"
FAULTS='illegal memory access|Memory access fault|HSA_STATUS_ERROR|Segmentation fault|Aborted'
has() { [[ " $STEPS " == *" $1 "* ]]; }
step() {  # $1 = name, $2 = rc, rest = the step's logs (files or directories)
  local name=$1 rc=$2; shift 2
  echo "$name rc=$rc"
  if [ "$rc" -ne 0 ] && [ "$rc" -ne 1 ]; then echo "stopping after $name"; exit "$rc"; fi
  if [ $# -gt 0 ] && grep -rqsE "$FAULTS" "$@"; then
    echo "stopping after $name: GPU fault text in its log:"
    grep -rsE -m 3 "$FAULTS" "$@" | cut -c1-300
    [ "$rc" -ne 0 ] && exit "$rc"
    exit 2
  fi
}
bench_line() {  # $1 = name, rest = bench.py arguments; the line goes to $O/$1.json
  local name=$1; shift
  timeout -k 10 300 python bench.py --full "$@" > $O/$name.log 2>&1
  local rc=$?
  step $name $rc $O/$name.log
  if [ $rc -ne 0 ]; then tail -5 $O/$name.log; exit $rc; fi
  tail -1 $O/$name.log > $O/$name.json
}
attribution() {  # $1 = trace directory, $2 = json, rest = step_attribution.py arguments
  local tr; tr=$(find $1 -name 'run_kernel_trace.csv' | head -1); local js=$2; shift 2
  [ -n "$tr" ] && python scripts/step_attribution.py "$tr" "$@" --json $js | tail -12
}
if has pytest; then
  SMCDET_PAIRED_OUT=$O/paired.json SMCDET_PAIRED_C5_OUT=$O/paired_c5.json SMCDET_C5_STATS_OUT=$O/c5_stats.json \
    timeout -k 10 ${TEST_LIMIT:-900} python -u -m pytest tests -m gpu -v -p no:cacheprovider --timeout 300 \
    --timeout-method thread ${PYTEST_ARGS:---ignore=tests/test_gpu_large_tile.py} \
    > $O/pytest_gpu.log 2>&1
  step pytest $? $O/pytest_gpu.log
  grep -E "^FAILED|passed|failed" $O/pytest_gpu.log | tail -12
fi
if has smoke; then
  timeout -k 10 300 python __graft_entry__.py smoke > $O/smoke.log 2>&1
  step smoke $? $O/smoke.log
  tail -2 $O/smoke.log
fi
if has bench; then
  timeout -k 10 400 python bench.py --full > $O/bench.log 2>&1
  step bench $? $O/bench.log
  tail -c 700 $O/bench.log; echo
fi
if has torchrun1; then
  timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 \
    --master-addr 127.0.0.1 --master-port 29531 bench.py --gpus 1 --full > $O/bench_torchrun1.log 2>&1
  step torchrun1 $? $O/bench_torchrun1.log
  tail -c 400 $O/bench_torchrun1.log; echo
fi
if has gloo2; then
  SMCDET_DIST_BACKEND=gloo timeout -k 10 300 python -m torch.distributed.run --nnodes=1 \
    --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --gpus 2 --full --steps 5 \
    --warmup 1 --no-cpu-baseline --no-full-run --no-vs-ref > $O/bench_gloo2.log 2>&1
  step gloo2 $? $O/bench_gloo2.log
  tail -1 $O/bench_gloo2.log
fi
if has lines; then  # unlike a failing test, a failing line ends the pass
  bench_line c2
  bench_line c3_64tiles --total-tiles 64 --no-cpu-baseline
  bench_line c3_9tiles --tiles-per-gpu 9 --no-cpu-baseline --no-vs-ref  # ~ a C3 rank share (64 tiles / 8 GPUs), square grid
  bench_line c4 --workload c4 --no-cpu-baseline
  bench_line c5 --workload c5 --no-cpu-baseline
  bench_line mcmc --workload mcmc
  bench_line mala --kernel mala --no-cpu-baseline
  bench_line agg --workload agg --no-cpu-baseline
fi
if has host; then  # host-side issue cost of a step vs its GPU time
  timeout -k 10 200 python scripts/host_overhead.py > $O/host_overhead.json 2>$O/host_overhead.err
  step host $? $O/host_overhead.err
  cat $O/host_overhead.json
fi
if has probe; then
  [ -x scripts/probe/issue_probe ] || /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 \
    -o scripts/probe/issue_probe scripts/probe/issue_probe.hip
  timeout -k 10 120 ./scripts/probe/issue_probe > $O/issue_probe.txt 2>&1
  step probe $? $O/issue_probe.txt
  cat $O/issue_probe.txt
fi
if has law; then
  timeout -k 10 600 python -u scripts/c2_law.py ${LAW_RUNS:-8192} > $O/c2_law.json 2> $O/c2_law.err
  step law $? $O/c2_law.err
  python -c "import json; d=json.load(open('$O/c2_law.json')); print({n: {k: (round(d[n][k]['rel_diff'], 5), [round(x, 5) for x in d[n][k]['rel_diff_95']]) for k in ('logZ', 'final_ess', 'iters')} for n in ('vs_oracle', 'vs_reference')})"
fi
if has paired; then  # -s: every seed's line reaches the log as it is written
  SMCDET_PAIRED_ALL=1 SMCDET_PAIRED_NO_TWIN=${NO_TWIN:-1} SMCDET_PAIRED_CHUNKS=${CHUNKS:-48} \
    SMCDET_PAIRED_PART=${PART:-} \
    SMCDET_PAIRED_OUT=$O/paired_all.json timeout -k 10 ${PAIRED_LIMIT:-3000} \
    python -u -m pytest tests/test_gpu_paired.py -s -q -p no:cacheprovider --timeout 600 \
    --timeout-method thread > $O/paired_all.log 2>&1
  step paired $? $O/paired_all.log
  tail -4 $O/paired_all.log
fi
if has profile; then
  OUT=$O/prof SUMMARY=$O/$PMC_SUMMARY SQ="$SQ" SQ2="$SQ2" SQ3="$SQ3" bash scripts/profile.sh
  step profile $? $O/prof
  tail -20 $O/prof/summary.txt
  attribution $O/prof/trace $O/step_attribution.json
fi
if has trace; then
  # the bench line's own command (prewarm on) under a kernel trace: the last
  # 20 steps' launches are the timed steps' identical replay, whose sweep /
  # tile durations the line reports as step_attribution -- the two must agree
  mkdir -p $O/trace_bench
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -T -f csv -d $O/trace_bench -o run -- \
    python3 bench.py --full --no-c3 --no-legs --no-vs-ref --no-full-run --no-cpu-baseline --no-spread \
    > $O/trace_bench.log 2>&1
  step trace $? $O/trace_bench.log
  attribution $O/trace_bench $O/trace_bench_attribution.json --tail 20
  grep '^{' $O/trace_bench.log | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('bench line:', json.dumps({k: d['step_attribution'][k] for k in ('sweep_ms', 'tile_pass_ms', 'timed_ms_per_step')}))"
fi
if has c4pmc; then
  OUT=$O/prof_c4 BENCH_ARGS="--workload c4" SQ="$SQ" SQ2="$SQ2" SQ3="$SQ3" PSTEPS=10 bash scripts/profile.sh
  step c4pmc $? $O/prof_c4
  python3 scripts/pmc_summary.py --root $O/prof_c4 --steps-per-launch 17203200 \
    --note "rocprofv3 passes of scripts/profile.sh over bench.py --workload c4 (42 8x8 cutouts, N=4096, K=100)" \
    --json $O/$PMC_SUMMARY_C4 > $O/prof_c4/summary.txt 2>&1
  tail -20 $O/prof_c4/summary.txt
fi
if has c5pmc; then
  # particle-steps per launch: 42 cutouts x 6 strata with s >= 1 x 8192 x 100
  OUT=$O/prof_c5 BENCH_ARGS="--workload c5" SQ="$SQ" SQ2="$SQ2" PSTEPS=10 bash scripts/profile.sh
  step c5pmc $? $O/prof_c5
  python3 scripts/pmc_summary.py --root $O/prof_c5 --steps-per-launch 206438400 \
    --note "rocprofv3 passes of scripts/profile.sh over bench.py --workload c5 (42 8x8 cutouts x 7 strata, N=8192, K=100)" \
    --json $O/$PMC_SUMMARY_C5 > $O/prof_c5/summary.txt 2>&1
  tail -20 $O/prof_c5/summary.txt
fi
if has postbench; then
  for f in $PMC_SUMMARY $PMC_SUMMARY_C4 $PMC_SUMMARY_C5; do
    [ -f $O/$f ] && cp $O/$f profiles/$f
  done
  timeout -k 10 400 python bench.py --full > $O/bench_post.log 2>&1
  step postbench $? $O/bench_post.log
  tail -c 400 $O/bench_post.log; echo
fi
if has large; then  # the global-memory (large-tile) paths, last
  timeout -k 10 300 python -u -m pytest tests/test_gpu_large_tile.py -v -p no:cacheprovider \
    --timeout 200 --timeout-method thread > $O/pytest_large.log 2>&1
  step large $? $O/pytest_large.log
  grep -E "^FAILED|passed|failed" $O/pytest_large.log | tail -8
fi
