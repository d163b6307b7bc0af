# Animator controllers on the device: parity on the GPU (tests/test_gpu_animators.py, with the IK and blend-stack tests behind it: the blend
# kernel is theirs), then tools/animator_time.py: 100 k Animators x 64 bones with a BLEND1D between two clips, the path fed from host records
# against lmx_animators_set_inputs + lmx_animators_update, alternating in one process. Every step under its own time limit; a step that
# fails ends the case. The results belong in profiles/animators/.
timeout -k 10 400 python -m pytest tests/test_gpu_animators.py tests/test_gpu_ik.py tests/test_animation.py -m gpu --durations=10 -x -q > "$OUT/animator_tests.log" 2>&1; rc=$?; echo "animator tests rc=$rc" | tee -a "$OUT/animator_tests.log"; tail -n 16 "$OUT/animator_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 400 python tools/animator_time.py --steps 20 --rounds 3 > "$OUT/animator_time.json" 2> "$OUT/animator_time.err"; rc=$?; echo "animator_time rc=$rc"; cat "$OUT/animator_time.json"; tail -n 5 "$OUT/animator_time.err"
[ $rc -eq 0 ] || return 1
