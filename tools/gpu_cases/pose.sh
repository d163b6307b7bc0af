# Pose processor: parity on the GPU (the 40-entity scene, then the lists that span waves, tiles and blocks), lmx_poses_run over 1 / 10 / 100 %
# of 100 k x 64 bones next to the skin run's pose kernel with the dual quaternions of every instance, then rocprofv3 kernel stats of the same
# tool in a run of its own
timeout 600 python -m pytest tests/test_gpu_pose_processor.py tests/test_gpu_pose_lists.py -m gpu --durations=10 -x -q > "$OUT/pose_tests.log" 2>&1; rc=$?; echo "pose tests rc=$rc" | tee -a "$OUT/pose_tests.log"; tail -n 3 "$OUT/pose_tests.log"
[ $rc -eq 0 ] || return 1
timeout 400 python tools/pose_time.py --steps 20 > "$OUT/pose_time.json" 2> "$OUT/pose_time.err"; rc=$?; echo "pose_time rc=$rc"; cat "$OUT/pose_time.json"; tail -n 5 "$OUT/pose_time.err"
[ $rc -eq 0 ] || return 1
prof pose python "$ROOT/tools/pose_time.py" --steps 10
python - "$OUT/pose_kernel_stats.csv" <<'PY' | tee "$OUT/pose_kernels.txt"
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "k_pose_" in r["Name"]:
        print(f'{r["Name"][:70]:70s} calls {int(r["Calls"]):5d}  avg {float(r["AverageNs"]) / 1e3:9.2f} us  min {float(r["MinNs"]) / 1e3:9.2f} us')
PY
