# Inverse kinematics in the device blend stack: parity on the GPU (tests/test_gpu_ik.py, with the blend-stack tests of tests/test_animation.py
# behind it), then tools/ik_time.py: 100 k Animators x 64 bones, two SAMPLE layers, without IK through the old and the new entry, with two
# 3-bone chains and with one 16-bone chain, alternating in one process. Every step under its own time limit; a step that fails ends the case.
# The results belong in profiles/ik/, next to the CPU baseline (python tools/ik_time.py --reference, where the reference tree is).
timeout -k 10 400 python -m pytest tests/test_gpu_ik.py tests/test_animation.py -m gpu --durations=10 -x -q > "$OUT/ik_tests.log" 2>&1; rc=$?; echo "ik tests rc=$rc" | tee -a "$OUT/ik_tests.log"; tail -n 16 "$OUT/ik_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 400 python tools/ik_time.py --steps 20 --rounds 3 > "$OUT/ik_time.json" 2> "$OUT/ik_time.err"; rc=$?; echo "ik_time rc=$rc"; cat "$OUT/ik_time.json"; tail -n 5 "$OUT/ik_time.err"
[ $rc -eq 0 ] || return 1
