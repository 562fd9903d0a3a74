# One gpurun call: GPU tests, the bench line, one rank's share (125 heliostats), kernel stats of both.  usage: bash tools/r4_pass.sh <tag> [notests|"pytest -k expr"]
cd $GRAFT_REPO_ROOT
export OUT=${OUT:-$PWD/tools_out}; mkdir -p "$OUT"
tag=$1
if [ "$2" != "notests" ]; then
  timeout -k 10 1000 python -m pytest tests -m gpu -x -v --tb=short --timeout 240 --durations=12 ${2:+-k "$2"} > $OUT/${tag}_gpu_tests.log 2>&1
  grep -E "FAILED|ERROR|Timeout| passed| failed|^E  " $OUT/${tag}_gpu_tests.log | cut -c1-300 | tail -15
fi
timeout -k 10 300 python tools/nurbs_bench.py 1000 125 2> $OUT/${tag}_nurbs_bench.err | tail -1 > $OUT/${tag}_nurbs_bench.json; cat $OUT/${tag}_nurbs_bench.json; tail -3 $OUT/${tag}_nurbs_bench.err
timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline > $OUT/${tag}_bench.log 2>&1; tail -1 $OUT/${tag}_bench.log > $OUT/${tag}_bench.json; cut -c1-600 $OUT/${tag}_bench.json
timeout -k 10 300 python bench.py --heliostats 125 --steps 30 --warmup 5 --full --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/${tag}_bench_h125.json; cut -c1-600 $OUT/${tag}_bench_h125.json
timeout -k 10 300 python tools/pipeline_probe.py 125 1 2 3 4 > $OUT/${tag}_pipeline_probe.txt 2>&1; tail -5 $OUT/${tag}_pipeline_probe.txt
bash tools/kstats.sh ${tag} > $OUT/${tag}_kstats.txt 2>&1 || true
bash tools/kstats.sh ${tag}125 --heliostats 125 > $OUT/${tag}_kstats_h125.txt 2>&1 || true
python tools/gap_report.py $OUT/ks_${tag}125 8 > $OUT/${tag}_gap_h125.txt 2>&1 || true
cat $OUT/${tag}_kstats.txt $OUT/${tag}_kstats_h125.txt $OUT/${tag}_gap_h125.txt
echo done
