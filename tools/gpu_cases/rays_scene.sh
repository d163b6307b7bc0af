# Procedural geometry and terrains in the cast: parity on the GPU (tests/test_gpu_rays_scene.py), the span of a whole castRay over the scene
# of rays_im.sh plus one 2048 x 2048 terrain and 64 procedural geometries for batches of 1 / 1024 / 65 536 rays warm and behind a scrub,
# with the same cast's span once both tables are cleared, then rocprofv3 kernel stats of the same tool in runs of their own. Every step
# under its own time limit; a step that fails ends the case. The results belong in profiles/rays/.
timeout -k 10 600 python -m pytest tests/test_gpu_rays_scene.py -m gpu --durations=10 -x -q > "$OUT/ray_scene_tests.log" 2>&1; rc=$?; echo "ray scene tests rc=$rc" | tee -a "$OUT/ray_scene_tests.log"; tail -n 3 "$OUT/ray_scene_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 500 python tools/ray_scene_time.py --steps 20 > "$OUT/ray_scene_time.json" 2> "$OUT/ray_scene_time.err"; rc=$?; echo "ray_scene_time rc=$rc"; cat "$OUT/ray_scene_time.json"; tail -n 5 "$OUT/ray_scene_time.err"
[ $rc -eq 0 ] || return 1
for n in 1 1024 65536; do # per-kernel times, one batch size per run
	prof rays_scene_$n python "$ROOT/tools/ray_scene_time.py" --steps 5 --rays $n --plain 0
	[ -f "$OUT/rays_scene_${n}_kernel_stats.csv" ] || return 1 # (the run left no stats: nothing more is started)
	python - "$OUT/rays_scene_${n}_kernel_stats.csv" $n <<'PY' | tee -a "$OUT/ray_scene_kernels.txt"
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if any(k in r["Name"] for k in ("k_pgray_", "k_terrain_", "k_ray_", "k_imray_")):
        print(f'{sys.argv[2]:>7s} rays  {r["Name"][:60]:60s} calls {int(r["Calls"]):5d}  avg {float(r["AverageNs"]) / 1e3:9.2f} us  min {float(r["MinNs"]) / 1e3:9.2f} us')
PY
done
