set -o pipefail
# usage (GPU box): bash tools/round_run.sh <tag>   -- GPU test suite, bench line (timed), kernel trace of the bench
# (logs and the bench line go to $RUN_DIR, default runs/)
tag=${1:-r2}
out=${RUN_DIR:-runs}
mkdir -p "$out"
timeout -k 10 1000 python -m pytest tests -q -m gpu -x > "$out/${tag}_tests.log" 2>&1; rc=$?; tail -5 "$out/${tag}_tests.log"; [ $rc -eq 0 ] || exit $rc
t0=$SECONDS
timeout -k 10 900 python bench.py --full > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err" || { tail -5 "$out/${tag}_bench.err"; exit 1; }
echo "bench wall $((SECONDS - t0)) s" | tee "$out/${tag}_bench_wall.txt"
cut -c1-300 "$out/${tag}_bench.json"
bash tools/kernel_trace.sh ${tag}_bench_trace bench.py --full --steps 50 --warmup 5 --no-cpu 2> /dev/null | sed -n 1,12p; echo trace rc=$?
