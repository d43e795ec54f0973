#!/bin/bash
OUT=${OUT:-out}       # where the logs and JSON lines go
mkdir -p $OUT
python __graft_entry__.py smoke > $OUT/smoke.log 2>&1; echo "smoke rc=$?"; tail -1 $OUT/smoke.log
bash profiles/collect.sh r01m > $OUT/collect.log 2>&1; echo "collect rc=$?"; tail -5 $OUT/collect.log
timeout -k 10 400 python bench.py --full > $OUT/default_bench.json 2> $OUT/default_bench.err; echo "default bench rc=$?"; tail -c 600 $OUT/default_bench.json
