#!/bin/bash
# Round 4 evidence on the GPU box (through gpurun): the bench line as the driver runs it, the GPU tests, smoke, kernel traces
# (stream and near-lone), the pipeline timeline and stage clocks, PMC passes at FULL config 3, ns/row of the row sweep against the
# anti-diagonal prototype, chain-extraction phase profile, and the N = 2 code path on one GPU (weak and strong scaling flags).
#   bash tools/prof_round4.sh [outdir]
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
OUT=${1:-gpurun_out/r04_final}
mkdir -p $OUT
WL=/dev/shm/mpa_wl
(time python bench.py --steps 20 --warmup 5 --full --workload-cache $WL) > $OUT/bench.json 2> $OUT/bench.err; python tools/bench_line.py $OUT/bench.json "bench (driver settings)"
(time python -m pytest tests -m gpu -q) > $OUT/pytest_gpu.log 2>&1; grep -h "passed\|failed" $OUT/pytest_gpu.log | tail -2
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; tail -1 $OUT/smoke.log | cut -c1-100
# kernel trace of the bench command (shorter job)
rm -rf $OUT/trace; rocprofv3 --kernel-trace --stats -d $OUT/trace -o t -- python bench.py --no-extra --no-cpu-baseline --no-cli --steps 5 --warmup 1 --workload-cache $WL > $OUT/trace_bench.json 2> $OUT/trace.err
DB=$(find $OUT/trace -name "t_results.db" | head -1)
python tools/rocpd_stats.py $DB > $OUT/kernel_trace_stats.txt 2>&1; head -9 $OUT/kernel_trace_stats.txt | cut -c1-140
python tools/timeline.py $DB 2500 60 > $OUT/dispatch_timeline.txt 2>&1
rm -rf $OUT/trace
# the same kernels nearly alone
rm -rf $OUT/trace; MPA_DP_LANES=1 MPA_SEEDERS=1 MPA_PLANNERS=1 rocprofv3 --kernel-trace --stats -d $OUT/trace -o t -- python bench.py --no-extra --no-cpu-baseline --no-cli --steps 2 --warmup 1 --workload-cache $WL > $OUT/trace_lone_bench.json 2>> $OUT/trace.err
DB=$(find $OUT/trace -name "t_results.db" | head -1)
python tools/rocpd_stats.py $DB > $OUT/kernel_trace_stats_lone.txt 2>&1
rm -rf $OUT/trace
# pipeline timeline + stage clocks + chain-extraction phases
MPA_TRACE=1 MPA_TIMING=1 python bench.py --no-extra --no-cpu-baseline --no-cli --steps 5 --warmup 1 --workload-cache $WL > $OUT/gantt_bench.json 2> $OUT/gantt.err
python tools/gantt.py $OUT/gantt.err > $OUT/pipeline_gantt.txt 2>&1; head -16 $OUT/pipeline_gantt.txt
{ python tools/timing_agg.py < $OUT/gantt.err; grep "mpa-cpu" $OUT/gantt.err | tail -12; } > $OUT/stage_clocks.txt
MPA_TIMING=2 MPA_SEEDERS=1 python bench.py --no-extra --no-cpu-baseline --no-cli --steps 1 --warmup 1 --workload-cache $WL > /dev/null 2> $OUT/extract.err
grep "extract-prof" $OUT/extract.err | tail -8 > $OUT/chain_extract_phases.txt; cat $OUT/chain_extract_phases.txt
# ns/row: row sweep against the anti-diagonal prototype
{
echo "# ns/row: row sweep (ext_narrow<32>, production) vs anti-diagonal prototype (dp_antidiag.hip), right-extension calls"
echo "# lone wave: 4 calls = one wave; saturated: 16384 calls = 4096 waves (4 per SIMD)"
for AD in 0 1; do
  python tools/time_wide.py 32 20000 4 4 $AD | tail -1
  python tools/time_wide.py 24 20000 4 4 $AD | tail -1
  python tools/time_wide.py 32 4000 16384 4 $AD | tail -1
done
} > $OUT/antidiag_ns_per_row.txt 2>&1; cat $OUT/antidiag_ns_per_row.txt
# PMC at full config 3, one lane / seeder / planner (counters serialise the kernels anyway)
export PMC_CMD="python bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-extra --no-cli --workload-cache $WL"
export PMC_WORKLOAD_NOTE="config 3 at FULL size (3 Gbp x 20 000 proteins, -I -u, 4 000-protein mini-batches, two DP rounds per batch), 2 passes over the workload, MPA_DP_LANES=1 MPA_SEEDERS=1 MPA_PLANNERS=1"
bash tools/pmc_round.sh $OUT/pmc > $OUT/pmc.log 2>&1
find $OUT/pmc -name "*.db" -delete; find $OUT/pmc -type d -empty -delete
python - $OUT/pmc/pmc_summary.json <<'PY'
import json,sys
try:
    d=json.load(open(sys.argv[1]))
    for kn in ("k_dp_round","k_chain_extract","k_seed_sift<4096>","k_prep_rows","k_refine_scan_map"):
        k=d["kernels"].get(kn,{})
        print("PMC", kn, {x:(round(k[x],4) if isinstance(k.get(x),float) else k.get(x)) for x in ("avg_us","hbm_bytes_per_launch","hbm_gb_per_s","avg_resident_waves_per_simd","valu_issue_share_of_wave_cycles","lds_bank_conflict_rate")})
except Exception as e: print("pmc summary:", repr(e)[:200])
PY
# the N = 2 code path with both ranks on this one GPU (gloo; NOT a scaling number): identity at N > 1, dynamic deal, both scaling modes
for SC in weak strong; do
  ( HSA_ENABLE_IPC_MODE_LEGACY=0 timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29655 bench.py --gpus 2 --debug-shared-gpu --full --scaling $SC --batch 1000 --steps 1 --warmup 1 --no-extra --no-cli --threads 8 --workload-cache $WL ) > $OUT/bench_n2_shared_gpu_debug_$SC.json 2> $OUT/n2_$SC.err
  python tools/bench_line.py $OUT/bench_n2_shared_gpu_debug_$SC.json "N=2 shared GPU (debug, $SC)"
  tail -2 $OUT/n2_$SC.err | cut -c1-200
done
bash tools/hostinfo.sh > $OUT/hostinfo.txt 2>&1; head -3 $OUT/hostinfo.txt
rm -f $OUT/*.err $OUT/pmc/*.err
rm -rf $WL
du -sh $OUT
