# Draw runs + instance buffers: parity on the GPU, the dense 10 M workload's chain keys -> sort -> draw timed warm and behind a scrub,
# then rocprofv3 kernel stats of the same workload in a run of its own
timeout 900 python -m pytest tests/test_gpu_draw_commands.py tests/test_gpu_draw_boundaries.py -m gpu -x -q > "$OUT/draw_tests.log" 2>&1; rc=$?; echo "draw tests rc=$rc" | tee -a "$OUT/draw_tests.log"; tail -n 3 "$OUT/draw_tests.log"
[ $rc -eq 0 ] || return 1
timeout 400 python tools/draw_time.py --steps 20 > "$OUT/draw_time.json" 2> "$OUT/draw_time.err"; rc=$?; echo "draw_time rc=$rc"; cat "$OUT/draw_time.json"
[ $rc -eq 0 ] || return 1
prof draw python "$ROOT/tools/draw_time.py" --steps 10
python - "$OUT/draw_kernel_stats.csv" <<'PY' | tee "$OUT/draw_kernels.txt"
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "k_draw_" in r["Name"] or "k_keys_" in r["Name"] or "DeviceScan" in r["Name"] or "scan" in r["Name"].lower():
        print(f'{r["Name"][:70]:70s} calls {int(r["Calls"]):5d}  avg {float(r["AverageNs"]) / 1e3:9.2f} us  min {float(r["MinNs"]) / 1e3:9.2f} us')
PY
