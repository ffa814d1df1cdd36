ROOT=${ROOT:-$(pwd)}
OUT=${OUT:-$ROOT/results}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
DEJAVU_ROCTX=1 rocprofv3 --marker-trace --kernel-trace --stats --output-format csv -d $OUT/roctx -- python3 $ROOT/bench.py --full --gpus 1 --force-dist --steps 30 --warmup 5 --views 50000 --sensor 64 --headings 16 --cpu-views 0 > $OUT/suite/roctx_bench.json 2> $OUT/suite/roctx.err
echo roctx rc=$?
ls $OUT/roctx/*/; cat $OUT/roctx/*/*domain_stats.csv; head -5 $OUT/roctx/*/*marker*stats*.csv 2>/dev/null
python3 -c "
import json
d=json.loads(open('$OUT/suite/roctx_bench.json').read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['config']['exchange'])
"
