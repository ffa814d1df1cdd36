ROOT=${ROOT:-$(pwd)}
OUT=${OUT:-$ROOT/results}
mkdir -p "$OUT"
cd $ROOT
mkdir -p $OUT/suite $OUT/tune
timeout -k 10 1100 python -m pytest tests -m gpu -q -x > $OUT/suite/pytest.log 2>&1
rc=$?
tail -8 $OUT/suite/pytest.log
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 400 python bench.py --full --steps 30 --warmup 5 --cpu-views 0 --secondary 0 --batch-agents 32 > $OUT/tune/agent.json 2> $OUT/tune/agent.err
python -c "
import json
d=json.loads(open('$OUT/tune/agent.json').read().strip().splitlines()[-1])
print('agent', d['agent']['nav_steps_per_s'], d['agent']['nav_steps_per_s_fake'], d['agent']['ensemble_of_32_nav_steps_per_s'], d['agent']['median_step_us_and_steps_over_4x_median'])
print('ensemble', d.get('ensemble'))
"
