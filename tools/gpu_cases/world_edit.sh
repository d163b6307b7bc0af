# World edits on the device: parity on the GPU (tests/test_gpu_world_edit.py, tests/test_gpu_world_sync_edit_run.py), then tools/world_edit_time.py: config 3's hierarchy (1 M
# entities, 250 k roots x depth 4) with culling bindings and the moved list on, lmx_world_edit (one re-parenting; 1 k destroys + 1 k
# creates + 1 k re-parentings) against the unchanged lmx_world_set_parent in one process, then rocprofv3 kernel stats of the same tool in
# a run of its own. Every step under its own time limit; a step that fails ends the case. The results belong in profiles/world_edit/.
timeout -k 10 300 python -m pytest tests/test_gpu_world_edit.py tests/test_gpu_world_sync_edit_run.py -m gpu --durations=10 -x -q > "$OUT/world_edit_tests.log" 2>&1; rc=$?; echo "world edit tests rc=$rc" | tee -a "$OUT/world_edit_tests.log"; tail -n 3 "$OUT/world_edit_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 400 python tools/world_edit_time.py --steps 5 --rounds 3 > "$OUT/world_edit_time.json" 2> "$OUT/world_edit_time.err"; rc=$?; echo "world_edit_time rc=$rc"; cat "$OUT/world_edit_time.json"; tail -n 5 "$OUT/world_edit_time.err"
[ $rc -eq 0 ] || return 1
prof world_edit python "$ROOT/tools/world_edit_time.py" --steps 3 --rounds 1
[ -f "$OUT/world_edit_kernel_stats.csv" ] || return 1 # (the run left no stats: nothing more is started)
python - "$OUT/world_edit_kernel_stats.csv" <<'PY' | tee "$OUT/world_edit_kernels.txt"
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "k_edit_" in r["Name"] or "DeviceRadixSort" in r["Name"] or "DeviceScan" in r["Name"] or "rocprim" in r["Name"]:
        print(f'{r["Name"][:70]:70s} calls {int(r["Calls"]):5d}  avg {float(r["AverageNs"]) / 1e3:9.2f} us  min {float(r["MinNs"]) / 1e3:9.2f} us  max {float(r["MaxNs"]) / 1e3:9.2f} us')
PY
