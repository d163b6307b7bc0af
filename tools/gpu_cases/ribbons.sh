# Ribbon emitters on the device: parity on the GPU (tests/test_gpu_ribbons.py, then the particle tests they share kernels with), then
# tools/ribbon_time.py: trails, many systems x 1 emitter x 16 ribbons x 64 points. Every step under its own time limit; a step that fails
# ends the case. The results belong in profiles/ribbons/ (there is no CPU baseline yet: tools/ribbon_time.py says what it needs).
timeout -k 10 300 python -m pytest tests/test_gpu_ribbons.py -m gpu --durations=10 -s -q > "$OUT/ribbon_tests.log" 2>&1; rc=$?; echo "ribbon tests rc=$rc" | tee -a "$OUT/ribbon_tests.log"; tail -n 16 "$OUT/ribbon_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 400 python -m pytest tests/test_gpu_particles.py -m gpu -q > "$OUT/particle_tests.log" 2>&1; rc=$?; echo "particle tests rc=$rc" | tee -a "$OUT/particle_tests.log"; tail -n 6 "$OUT/particle_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 300 python tools/ribbon_time.py --steps 20 > "$OUT/ribbon_time.json" 2> "$OUT/ribbon_time.err"; rc=$?; echo "ribbon_time rc=$rc"; cat "$OUT/ribbon_time.json"; tail -n 5 "$OUT/ribbon_time.err"
[ $rc -eq 0 ] || return 1
