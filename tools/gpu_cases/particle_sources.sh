# MESH and SPLINE of the particle VM on the device: parity on the GPU (tests/test_gpu_particle_sources.py, then the ribbon and particle
# tests that share the kernels), then tools/particle_source_time.py: many systems on one skinned model, three MESH per particle and step,
# one SPLINE per particle and fill, against the same programs with MOV in their place. Every step under its own time limit; a step that
# fails ends the case. The results belong in profiles/particle_sources/.
timeout -k 10 300 python -m pytest tests/test_gpu_particle_sources.py -m gpu --durations=10 -s -q > "$OUT/source_tests.log" 2>&1; rc=$?; echo "source tests rc=$rc" | tee -a "$OUT/source_tests.log"; tail -n 16 "$OUT/source_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 300 python -m pytest tests/test_gpu_ribbons.py -m gpu -q > "$OUT/ribbon_tests.log" 2>&1; rc=$?; echo "ribbon tests rc=$rc" | tee -a "$OUT/ribbon_tests.log"; tail -n 6 "$OUT/ribbon_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 400 python -m pytest tests/test_gpu_particles.py -m gpu -q > "$OUT/particle_tests.log" 2>&1; rc=$?; echo "particle tests rc=$rc" | tee -a "$OUT/particle_tests.log"; tail -n 6 "$OUT/particle_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 300 python tools/particle_source_time.py --steps 20 > "$OUT/particle_source_time.json" 2> "$OUT/particle_source_time.err"; rc=$?; echo "particle_source_time rc=$rc"; cat "$OUT/particle_source_time.json"; tail -n 5 "$OUT/particle_source_time.err"
[ $rc -eq 0 ] || return 1
