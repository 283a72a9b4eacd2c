#!/bin/bash
# GPU session: new config tests, then bench.py N>1 rehearsals (ranks share
# cuda:0, gloo) at N=2 and N=4, then the N=1 bench, every line with --full.
# Stops at the first hard failure.  Output: $OUT_DIR (default bench_out/).
set -u
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R"
O="$R/${OUT_DIR:-bench_out}"
mkdir -p "$O"
export TMPDIR=/tmp HSA_ENABLE_IPC_MODE_LEGACY=0
TAG=${TAG:-r02}
timeout -k 10 400 python -u -m pytest -x -v --timeout 300 --timeout-method thread tests/test_gpu_configs.py ${PYTEST_ARGS:-} > "$O/pytest_cfg_$TAG.log" 2>&1
rc=$?; echo "pytest rc=$rc"; tail -15 "$O/pytest_cfg_$TAG.log"; [ $rc -ne 0 ] && exit $rc
for n in 2 4; do
  timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node $n --master-addr 127.0.0.1 --master-port 2950$n \
     bench.py --gpus $n --rehearse --full --steps 10 --warmup 3 > "$O/rehearse_${TAG}_$n.json" 2> "$O/rehearse_${TAG}_$n.err"
  rc=$?; echo "rehearse N=$n rc=$rc"; cat "$O/rehearse_${TAG}_$n.json"; [ $rc -ne 0 ] && { tail -30 "$O/rehearse_${TAG}_$n.err"; exit $rc; }
done
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 > "$O/bench_$TAG.json" 2> "$O/bench_$TAG.err"
rc=$?; echo "bench rc=$rc"; cat "$O/bench_$TAG.json"; [ $rc -ne 0 ] && { tail -20 "$O/bench_$TAG.err"; exit $rc; }
echo done
