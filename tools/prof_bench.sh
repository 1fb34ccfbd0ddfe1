#!/bin/bash
# Regenerates the bench artefacts under $OUT (default prof_out/; tools/pmc_summary.py then writes the summaries into profiles/):
#   bench line (default workload), rocprofv3 kernel stats (CSV), three PMC passes over the default workload (FETCH_SIZE;
#   WRITE_SIZE; TCC_HIT_sum + TCC_MISS_sum: separate passes, no trace flags).  FLASH-BS workloads: tools/prof_beam_pmc.sh.
#   Every bench.py call runs with --full: the profiles and traffic.json cover the sparse walk and the FLASH-BS extra too.
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-prof_out}
mkdir -p "$OUT" && rm -rf "$OUT/prof_bench" "$OUT/pmc1" "$OUT/pmc2" "$OUT/pmc3"
timeout -k 10 500 python3 bench.py --full > "$OUT/bench_n1.json" 2> "$OUT/bench_n1.err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_bench" -o bench -- python3 bench.py --full --steps 10 --no-cpu-baseline > "$OUT/prof_bench.log" 2>&1 &&
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc1" -o pmc -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/pmc1.log" 2>&1 &&
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc2" -o pmc -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/pmc2.log" 2>&1 &&
timeout -k 10 300 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d "$OUT/pmc3" -o pmc -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/pmc3.log" 2>&1
