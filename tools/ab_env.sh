#!/bin/bash
# A/B of an environment switch on the tree's build: tools/ab_env.sh VAR=VALUE  (driver's arguments x 3, 400 scans x 1)
# (log: $OUT_DIR/ab_env.log, OUT_DIR defaults to out)
out=${OUT_DIR:-out}; mkdir -p $out; rm -f $out/ab_env.log
pr='import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d["value"], d["ms_per_step"], d["config"].get("replay_matches_prepass"), d.get("api_scans_per_sec"))'
for rep in 1 2 3; do
  for v in "X_NONE=1" "$1"; do
    echo "== $v steps 20" >> $out/ab_env.log
    env $v python bench.py --full --steps 20 --warmup 5 --sectors 0 --cpu-scans 0 --pmc off 2>/dev/null | python -c "$pr" >> $out/ab_env.log 2>&1
  done
done
for v in "X_NONE=1" "$1"; do
  echo "== $v steps 400" >> $out/ab_env.log
  env $v python bench.py --full --steps 400 --warmup 20 --sectors 0 --cpu-scans 0 --pmc off 2>/dev/null | python -c "$pr" >> $out/ab_env.log 2>&1
done
cat $out/ab_env.log
