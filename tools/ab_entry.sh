#!/bin/bash
# A/B of two library builds at the driver's arguments and over 400 scans: libmht_amd.so.base (MHT_LIB_VARIANT=.base) against the tree's build
# (log: $OUT_DIR/ab.log, OUT_DIR defaults to out)
out=${OUT_DIR:-out}; mkdir -p $out
for rep in 1 2 3; do
  for v in .base ""; do
    echo "== variant '$v' steps 20" >> $out/ab.log
    MHT_LIB_VARIANT=$v python bench.py --full --steps 20 --warmup 5 --sectors 0 --cpu-scans 0 --pmc off 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d.get('stage_ms'), d.get('api_scans_per_sec'))" >> $out/ab.log 2>&1
  done
done
for v in .base ""; do
  echo "== variant '$v' steps 400" >> $out/ab.log
  MHT_LIB_VARIANT=$v python bench.py --full --steps 400 --warmup 20 --sectors 0 --cpu-scans 0 --pmc off 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d.get('stage_ms'), d.get('api_scans_per_sec'))" >> $out/ab.log 2>&1
done
cat $out/ab.log
