# Frame time vs scene size at 4096^2 (bench.py --full for the per-kernel
# times, N=1, no extras).  Output: $OUT_DIR (default bench_out/).
set -u
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R"
O="$R/${OUT_DIR:-bench_out}"
mkdir -p "$O"
for spec in "256 64 6.4" "1024 256 6.4" "4096 1024 6.4" "16384 4096 6.4" "4096 1024 1" "16384 4096 1" "65536 8192 1"; do
  set -- $spec
  J="$O/scale_$1_$2_$3"
  timeout -k 10 120 python bench.py --full --spheres $1 --cubes $2 --k $3 --steps 20 --warmup 3 --no-cpu-baseline --no-host-path --no-extras > "$J.json" 2> "$J.err"
  rc=$?; [ $rc -ne 0 ] && { echo "$spec rc=$rc"; tail -5 "$J.err"; exit $rc; }
  python -c "import json, sys; l=json.load(open(sys.argv[1])); r=l['roofline']; print('$1 spheres $2 cubes k=$3:', l['ms_per_step'], 'ms', l['value'], 'Mrays/s', 'prep', r['prep_ms'], 'bin', r['bin_ms'], 'trace', r['kernel_ms'], 'frac', r['frac'])" "$J.json"
done
