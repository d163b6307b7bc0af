# Instanced models: parity on the GPU (the -k instanced subset, full size included), the 10 M / 16-model workload timed warm and cold,
# then rocprofv3 kernel stats of the same workload in a run of its own
timeout 900 python -m pytest tests/test_gpu_instanced_models.py -m gpu -x -q > "$OUT/im_tests.log" 2>&1; rc=$?; echo "im tests rc=$rc" | tee -a "$OUT/im_tests.log"; tail -n 3 "$OUT/im_tests.log"
[ $rc -eq 0 ] || return 1
timeout 400 python tools/im_time.py --steps 20 > "$OUT/im_time.json" 2> "$OUT/im_time.err"; rc=$?; echo "im_time rc=$rc"; cat "$OUT/im_time.json"
[ $rc -eq 0 ] || return 1
prof im python "$ROOT/tools/im_time.py" --steps 10
python - "$OUT/im_kernel_stats.csv" <<'PY' | tee "$OUT/im_kernels.txt"
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "k_im_" in r["Name"]:
        print(f'{r["Name"][:60]:60s} calls {int(r["Calls"]):5d}  avg {float(r["AverageNs"]) / 1e3:9.2f} us  min {float(r["MinNs"]) / 1e3:9.2f} us')
PY
