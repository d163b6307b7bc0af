# fillClusters: parity on the GPU (hand-made lights, records, probes, the seeded 1920 x 1080 list, the chain behind a cull, overflow), the
# span of lmx_clusters_run over 1 k / 10 k / 100 k visible lights warm and behind a scrub, then rocprofv3 kernel stats of the same tool in a
# run of its own. Every step under its own time limit; a step that fails ends the case.
timeout -k 10 600 python -m pytest tests/test_gpu_clusters.py -m gpu --durations=10 -x -q > "$OUT/cluster_tests.log" 2>&1; rc=$?; echo "cluster tests rc=$rc" | tee -a "$OUT/cluster_tests.log"; tail -n 3 "$OUT/cluster_tests.log"
[ $rc -eq 0 ] || return 1
timeout -k 10 400 python tools/cluster_time.py --steps 20 > "$OUT/cluster_time.json" 2> "$OUT/cluster_time.err"; rc=$?; echo "cluster_time rc=$rc"; cat "$OUT/cluster_time.json"; tail -n 5 "$OUT/cluster_time.err"
[ $rc -eq 0 ] || return 1
for n in 1000 10000 100000; do # per-kernel times, one size per run
	prof cluster_$n python "$ROOT/tools/cluster_time.py" --steps 10 --lights $n
	[ -f "$OUT/cluster_${n}_kernel_stats.csv" ] || return 1 # (the run left no stats: nothing more is started)
	python - "$OUT/cluster_${n}_kernel_stats.csv" $n <<'PY' | tee -a "$OUT/cluster_kernels.txt"
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "k_cluster_" in r["Name"]:
        print(f'{sys.argv[2]:>7s} lights  {r["Name"][:60]:60s} calls {int(r["Calls"]):5d}  avg {float(r["AverageNs"]) / 1e3:9.2f} us  min {float(r["MinNs"]) / 1e3:9.2f} us')
PY
done
