# A/B of library variants on one box, interleaved, a plain bench.py process per run (bash):
#   ab_libs.sh OUTDIR REPS VARIANT...   (VARIANT = default | name of _build/var_NAME, scripts/build_variant.py)
# Per repetition: configs #2, #4, #3, each with every variant in the order given.  One JSON result line per
# run in OUTDIR/ab.jsonl, tagged with variant and repetition; stops at the first run that fails.
set -eo pipefail
OUT=$1; REPS=$2; shift 2; mkdir -p $OUT
for rep in $(seq 1 $REPS); do
for run in "config2 2000 200" "config4 200 50" "config3 50 20"; do
  read CFG STEPS WARM <<< "$run"
  for v in "$@"; do
    if [ "$v" = default ]; then LIB=""; else LIB=cyclonus_amd/_build/var_$v/libcyclonus_hip.so; fi
    CYC_HIP_LIB=$LIB timeout -k 10 300 python -u bench.py --gpus 1 --config $CFG --steps $STEPS --warmup $WARM 2> $OUT/ab_${CFG}_${v}_$rep.err \
      | tail -1 | sed "s/^{/{\"ab_variant\": \"$v\", \"ab_rep\": $rep, /" >> $OUT/ab.jsonl
  done
done
done
