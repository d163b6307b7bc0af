# castRayInstancedModels in the cast: parity on the GPU (tests/test_gpu_rays_im.py), the span of a cast over 1 M instances of four
# instanced models for batches of 1 / 1024 / 65 536 rays warm and behind a scrub, then rocprofv3 kernel stats of the same tool in runs of
# their own. Every step under its own time limit; a step that fails ends the case. The results belong in profiles/rays/.
timeout -k 10 600 python -m pytest tests/test_gpu_rays_im.py -m gpu --durations=10 -x -q > "$OUT/ray_im_tests.log" 2>&1; rc=$?; echo "ray im tests rc=$rc" | tee -a "$OUT/ray_im_tests.log"; tail -n 3 "$OUT/ray_im_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 500 python tools/ray_im_time.py --steps 20 > "$OUT/ray_im_time.json" 2> "$OUT/ray_im_time.err"; rc=$?; echo "ray_im_time rc=$rc"; cat "$OUT/ray_im_time.json"; tail -n 5 "$OUT/ray_im_time.err"
[ $rc -eq 0 ] || return 1
for n in 1 1024 65536; do # per-kernel times, one batch size per run
	prof rays_im_$n python "$ROOT/tools/ray_im_time.py" --steps 5 --rays $n --plain 0
	[ -f "$OUT/rays_im_${n}_kernel_stats.csv" ] || return 1 # (the run left no stats: nothing more is started)
	python - "$OUT/rays_im_${n}_kernel_stats.csv" $n <<'PY' | tee -a "$OUT/ray_im_kernels.txt"
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "k_imray_" in r["Name"] or "k_ray_" in r["Name"]:
        print(f'{sys.argv[2]:>7s} rays  {r["Name"][:60]:60s} calls {int(r["Calls"]):5d}  avg {float(r["AverageNs"]) / 1e3:9.2f} us  min {float(r["MinNs"]) / 1e3:9.2f} us')
PY
done
