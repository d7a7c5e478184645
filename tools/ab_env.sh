# same-box A/B of an environment knob on the bench (forward + training lines): usage ENVSET="K=V" bash tools/ab_env.sh
set -e
OUT=${TMAE_OUT_DIR:-bench_out}  # where logs, traces and profiles go
mkdir -p $OUT
for v in base knob base knob; do
  if [ $v = knob ]; then export $ENVSET; else unset ${ENVSET%%=*}; fi
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-k64 --no-roofline --steps 20 --warmup 5 > $OUT/abe_$v.log 2>&1
  grep '^{' $OUT/abe_$v.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('$v', d['value'], d.get('train',{}).get('value'))"
done
