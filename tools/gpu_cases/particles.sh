# Particle systems: parity on the GPU (tests/test_gpu_particles.py; its SIN / COS test prints the largest distance to libm, which belongs in
# DESIGN §4.15 and, doubled, in the test's bound), the span of one step plus fill for 256 emitters x 64 k particles warm and behind a scrub,
# then rocprofv3 kernel stats of the same tool in a run of its own. Every step under its own time limit; a step that fails ends the case.
# The results belong in profiles/particles/, next to the CPU baseline (python tools/particle_time.py --reference, where the reference tree is).
timeout -k 10 600 python -m pytest tests/test_gpu_particles.py -m gpu --durations=10 -x -q -s > "$OUT/particle_tests.log" 2>&1; rc=$?; echo "particle tests rc=$rc" | tee -a "$OUT/particle_tests.log"; grep "SIN / COS" "$OUT/particle_tests.log"; tail -n 3 "$OUT/particle_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 500 python tools/particle_time.py --steps 20 > "$OUT/particle_time.json" 2> "$OUT/particle_time.err"; rc=$?; echo "particle_time rc=$rc"; cat "$OUT/particle_time.json"; tail -n 5 "$OUT/particle_time.err"
[ $rc -eq 0 ] || return 1
prof particles python "$ROOT/tools/particle_time.py" --steps 5
[ -f "$OUT/particles_kernel_stats.csv" ] || return 1 # (the run left no stats: nothing more is started)
python - "$OUT/particles_kernel_stats.csv" <<'PY' | tee -a "$OUT/particle_kernels.txt"
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "k_particles_" in r["Name"]:
        print(f'{r["Name"][:70]:70s} calls {int(r["Calls"]):5d}  avg {float(r["AverageNs"]) / 1e3:9.2f} us  min {float(r["MinNs"]) / 1e3:9.2f} us')
PY
