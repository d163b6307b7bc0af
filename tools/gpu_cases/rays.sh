# castRay: parity on the GPU (hand-made triangles, flags, ties, the narrow phase's edges, skinning, transforms, the seeded scene, overflow,
# errors), the span of a cast over 1 M instances for batches of 1 / 1024 / 65 536 rays warm and behind a scrub, then rocprofv3 kernel stats
# of the same tool in runs of their own. Every step under its own time limit; a step that fails ends the case.
timeout -k 10 600 python -m pytest tests/test_gpu_rays.py -m gpu --durations=10 -x -q > "$OUT/ray_tests.log" 2>&1; rc=$?; echo "ray tests rc=$rc" | tee -a "$OUT/ray_tests.log"; tail -n 3 "$OUT/ray_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 500 python tools/ray_time.py --steps 20 > "$OUT/ray_time.json" 2> "$OUT/ray_time.err"; rc=$?; echo "ray_time rc=$rc"; cat "$OUT/ray_time.json"; tail -n 5 "$OUT/ray_time.err"
[ $rc -eq 0 ] || return 1
for n in 1 1024 65536; do # per-kernel times, one batch size per run
	prof rays_$n python "$ROOT/tools/ray_time.py" --steps 5 --rays $n
	[ -f "$OUT/rays_${n}_kernel_stats.csv" ] || return 1 # (the run left no stats: nothing more is started)
	python - "$OUT/rays_${n}_kernel_stats.csv" $n <<'PY' | tee -a "$OUT/ray_kernels.txt"
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "k_ray_" in r["Name"]:
        print(f'{sys.argv[2]:>7s} rays  {r["Name"][:60]:60s} calls {int(r["Calls"]):5d}  avg {float(r["AverageNs"]) / 1e3:9.2f} us  min {float(r["MinNs"]) / 1e3:9.2f} us')
PY
done
