# The animation sampler at its bit and clip-end edges, on the GPU: the two new files (tests/test_anim_edges.py pins the expected values on the
# CPU and asserts the cases' coverage, tests/test_gpu_anim_edges.py runs them through the three kernels), then the older animation and IK files
# that share the kernels. Each step under its own time limit; the first failing test ends its step, a failing step ends the case.
# The durations belong in profiles/anim/anim_tests.log.
timeout -k 10 400 python -m pytest tests/test_anim_edges.py tests/test_gpu_anim_edges.py --durations=0 --durations-min=0.02 -x -q > "$OUT/anim_tests.log" 2>&1; rc=$?; echo "anim edge tests rc=$rc" | tee -a "$OUT/anim_tests.log"; tail -n 25 "$OUT/anim_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 400 python -m pytest tests/test_animation.py tests/test_gpu_ik.py --durations=10 -x -q > "$OUT/anim_older_tests.log" 2>&1; rc=$?; echo "animation + ik tests rc=$rc" | tee -a "$OUT/anim_older_tests.log"; tail -n 16 "$OUT/anim_older_tests.log"
[ $rc -eq 0 ] || return 1
