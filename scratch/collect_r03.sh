#!/bin/bash
# round 3 evidence run: smoke, rocprofv3 passes (profiles/collect.sh <tag>), default bench with --full, secondary workloads
TAG=${1:-r03a}
OUT=${OUT:-out}       # where the logs and JSON lines go
mkdir -p $OUT
python __graft_entry__.py smoke > $OUT/${TAG}_smoke.log 2>&1; echo "smoke rc=$?"; tail -1 $OUT/${TAG}_smoke.log
bash profiles/collect.sh $TAG > $OUT/collect_$TAG.log 2>&1; echo "collect rc=$?"; tail -4 $OUT/collect_$TAG.log
timeout -k 10 500 python bench.py --full > $OUT/${TAG}_bench_default.json 2> $OUT/${TAG}_bench_default.err; echo "default bench rc=$?"
cp $OUT/${TAG}_bench_default.json profiles/${TAG}_bench_default.json
: > $OUT/${TAG}_secondary.jsonl
for args in "--workload ffhq_sg2" "--workload big_gan" "--workload sg2attent" "--workload sg2attent --res 256" "--ada 0.5" "--num-fp16-res 0"; do
  timeout -k 10 400 python bench.py --full $args --no-cpu-baseline --no-secondary >> $OUT/${TAG}_secondary.jsonl 2>> $OUT/${TAG}_secondary.err || echo "FAILED: $args" >> $OUT/${TAG}_secondary.jsonl
  echo "done: $args"
done
cp $OUT/${TAG}_secondary.jsonl profiles/${TAG}_secondary_workloads.jsonl
mkdir -p $OUT/profiles_out && cp profiles/${TAG}_* $OUT/profiles_out/
python - $TAG $OUT <<'PY'
import json, sys
tag, out = sys.argv[1:3]
r = json.load(open(f'{out}/{tag}_bench_default.json'))
print({k: r[k] for k in ('value', 'ms_per_step', 'ms_per_step_median', 'target_kernel', 'sbg_kernel_time_frac_of_step')}, r['roofline']['frac'], [s_['value'] for s_ in r.get('secondary', [])], r['cpu_baseline']['value'])
for l in open(f'{out}/{tag}_secondary.jsonl'):
    try:
        d = json.loads(l); print(d['metric'], d['value'], d['ms_per_step'])
    except Exception: print(l.strip()[:100])
PY
