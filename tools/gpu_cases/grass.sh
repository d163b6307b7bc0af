# Terrain grass on the device: parity on the GPU (tests/test_gpu_grass.py; its last test prints the largest rotation difference of the run,
# the figure behind ROT_MEASURED), then tools/grass_time.py: 4 terrains x 4 types, the cut frame, the walk frame and the cull of five views.
# Every step under its own time limit; a step that fails ends the case. The results belong in profiles/grass/, next to the CPU baseline
# (python tools/grass_time.py --reference, where the reference tree is).
timeout -k 10 400 python -m pytest tests/test_gpu_grass.py -m gpu --durations=10 -s -q > "$OUT/grass_tests.log" 2>&1; rc=$?; echo "grass tests rc=$rc" | tee -a "$OUT/grass_tests.log"; tail -n 16 "$OUT/grass_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 300 python tools/grass_time.py --steps 5 --rounds 3 > "$OUT/grass_time.json" 2> "$OUT/grass_time.err"; rc=$?; echo "grass_time rc=$rc"; cat "$OUT/grass_time.json"; tail -n 5 "$OUT/grass_time.err"
[ $rc -eq 0 ] || return 1
