#!/bin/bash
# One evidence run on a GPU box (replaces the per-round gpu_rN_final.sh scripts): whole GPU suite, smoke, the bench lines (c2 default = fp32
# vocoder `value` + bf16x3 `split`, incl. live PMC and the CPU baseline; c3, c5, one / two clips, one stream), rocprofv3 kernel stats of the
# default / one-stream / one-clip commands per vocoder precision, SQ counter pass.  Everything lands in gpurun_out/<tag>/; copy what is
# quoted to profiles/<round>_*.
#   gpurun --timeout 3000 -- 'bash tools/gpu_evidence.sh r4z'
set -u
TAG=${1:-ev}
mkdir -p gpurun_out/$TAG
export TMPDIR=/tmp
R=$PWD
O=$R/gpurun_out/$TAG
if [ "${SKIP_TESTS:-0}" != "1" ]; then
timeout 2400 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > $O/gpu_tests.log 2>&1
echo "gpu tests exit: $?" >> $O/gpu_tests.log
tail -6 $O/gpu_tests.log
timeout 300 python __graft_entry__.py --smoke 2>&1 | tail -2 | tee $O/smoke.log
fi
timeout 900 python bench.py --full > $O/bench_c2.json 2> $O/bench_c2.err
timeout 400 python bench.py --full --workload c3 --steps 1 --warmup 1 --no-cpu-baseline > $O/bench_c3.json 2> $O/bench_c3.err
timeout 400 python bench.py --full --workload c5 --steps 1 --warmup 1 --no-cpu-baseline > $O/bench_c5.json 2> $O/bench_c5.err
timeout 300 python bench.py --full --batch 1 --streams 1 --steps 4 --warmup 2 --no-cpu-baseline --no-pmc > $O/bench_b1.json 2> $O/bench_b1.err
timeout 300 python bench.py --full --batch 2 --streams 1 --steps 4 --warmup 2 --no-cpu-baseline --no-pmc > $O/bench_b2.json 2> $O/bench_b2.err
timeout 300 python bench.py --full --streams 1 --steps 3 --warmup 1 --no-cpu-baseline --no-pmc > $O/bench_s1.json 2> $O/bench_s1.err
for f in c2 c3 c5 b1 b2 s1; do python - <<PY
import json
try:
    d=json.loads([l for l in open('$O/bench_$f.json') if l.startswith('{')][-1])
    sp=d.get('split') or {}
    print('$f', 'value', round(d['value'],1), 'ms', round(d['ms_per_step'],2), 'frac', round(d['roofline']['frac'],4), 'parity', d['parity_check'] and d['parity_check']['ok'],
          '| split', sp and round(sp['value'],1), sp and round(sp['ms_per_step'],2), sp and sp['parity_check'] and sp['parity_check']['ok'], d['device']['clocks_during_timed_region'].get('sclk_mhz_avg'))
    for r in d['roofline']['classes']+(sp.get('classes') or []): print('   ', r['class'][:44], round(r['ms_per_pass'],2), 'ms', round(r['avg_launch_us'],1),'us', round(r['frac_of_mfma_peak'],4), r['launches_per_pass'])
except Exception as e:
    print('$f', 'FAILED', e)
PY
done
cd /tmp
prof() { # name args passes
  timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$1 -o b -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-isolated --no-pmc --no-parity-check $2 > $O/$1.log 2>&1
  f=$(find $O/$1 -name "*kernel_stats.csv" | head -1)
  cp "$f" $O/${1}_kernel_stats.csv
  python $R/tools/prof_summary.py $O/${1}_kernel_stats.csv ${3:-2} 16
  find $O/$1 -name "*kernel_trace.csv" -delete
}
prof stream1_fp32 "--streams 1 --vocoder-precision fp32"
prof stream1_split "--streams 1 --vocoder-precision split"
prof batch1_fp32 "--streams 1 --batch 1 --vocoder-precision fp32"
prof batch1_split "--streams 1 --batch 1 --vocoder-precision split"
prof default_both "" 4
cd $R
bash tools/gpu_sq_pmc.sh $TAG --vocoder-precision fp32 2>&1 | tail -40
