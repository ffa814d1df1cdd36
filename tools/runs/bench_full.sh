ROOT=${ROOT:-$(pwd)}
OUT=${OUT:-$ROOT/results}
mkdir -p "$OUT"
cd $ROOT
mkdir -p $OUT/bench
DEJAVU_VERBOSE=1 timeout -k 10 900 python bench.py --full > $OUT/bench/full.json 2> $OUT/bench/full.err
echo rc=$?
tail -5 $OUT/bench/full.err
python -c "
import json
d=json.loads(open('$OUT/bench/full.json').read().strip().splitlines()[-1])
print(json.dumps(d, indent=1)[:6000])
"
