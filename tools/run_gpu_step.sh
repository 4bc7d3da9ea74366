# GPU check in one go: the GPU tier of the tests, the smoke check, the full bench line and a 2-rank rehearsal of the
# self-spawning bench (gloo: both ranks share the one GPU of the box).  Stops at the first step that fails.
# usage: bash tools/run_gpu_step.sh <output dir>
O=${1:?usage: bash tools/run_gpu_step.sh <output dir>}/step
mkdir -p "$O"
timeout -k 10 1100 python -m pytest tests -q -m gpu > "$O/pytest.log" 2>&1; rc=$?; tail -4 "$O/pytest.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$O/smoke.log" 2>&1; rc=$?; tail -1 "$O/smoke.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > "$O/bench.json" 2> "$O/bench.err"; rc=$?; echo "bench rc $rc"; tail -c 400 "$O/bench.json"; [ $rc -eq 0 ] || exit $rc
B4D_BENCH_BACKEND=gloo timeout -k 10 600 python bench.py --gpus 2 --frames 64 --steps 5 --full --no-cpu > "$O/bench2.json" 2> "$O/bench2.err"; rc=$?; echo "bench2 rc $rc"; tail -c 300 "$O/bench2.json"; exit $rc
