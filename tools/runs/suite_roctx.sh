ROOT=${ROOT:-$(pwd)}
OUT=${OUT:-$ROOT/results}
mkdir -p "$OUT"
cd $ROOT
mkdir -p $OUT/suite
timeout -k 10 1100 python -m pytest tests -m gpu -q > $OUT/suite/pytest.log 2>&1
rc=$?
tail -25 $OUT/suite/pytest.log
if [ $rc -ne 0 ]; then exit $rc; fi
# roctx ranges: a marker trace of a short agent + exchange run
cd /tmp && export TMPDIR=/tmp
DEJAVU_ROCTX=1 rocprofv3 --marker-trace --kernel-trace --stats --output-format csv -d $OUT/roctx -- python3 $ROOT/bench.py --full --gpus 1 --force-dist --steps 30 --warmup 5 --views 50000 --sensor 64 --headings 16 --cpu-views 0 > $OUT/suite/roctx_bench.json 2> $OUT/suite/roctx.err
echo roctx rc=$?
ls $OUT/roctx/*/ | head; tail -3 $OUT/suite/roctx.err
