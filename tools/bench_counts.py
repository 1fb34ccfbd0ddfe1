#!/usr/bin/env python3
"""bench_counts.py — fv_expected_counts beside fv_posteriors on the cfg2 model (K = 3965, T = 256), one sequence and 8
sequences.  One process; the measured calls are alternated, at least --min-seconds each, --alternations
times; medians and ranges.

  python tools/bench_counts.py [--min-seconds 0.5] [--alternations 5] [--parent-root DIR] [--bench-steps 20]
                               [--kernel-stats CSV] [--out profiles/counts_bench.json] [--git-head REV]

What it records, per alternation from the HIP-event time of the call (fv_counts_stats.gpu_ms, fv_sumprod_stats.gpu_ms):
  counts_ms[1 | 8]       fv_expected_counts with every output, trans_out on the host
  posteriors_ms[1 | 8]   fv_posteriors (no gamma_out) on the same sequences, one call each, summed
  counts_over_posteriors their ratio: what the counting kernels add to the two passes they follow
and the wall time per call of each.
--kernel-stats: the kernel_stats CSV of a separate
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_counts.py --trace-child
run (20 single-sequence calls and nothing else): the average time of every kernel of the call is copied into the JSON, and
counts_xi's is set against its two floors: bytes, 20 K^2 per launch (the float64
accumulator read and written, the float32 table read) at the HBM rate, and flops, 2 K^2 (T - 1) at the float64 vector rate
(half the float32 vector rate).
--parent-root: a built checkout of the parent commit; `python bench.py --gpus 1 --steps N` is run in child processes on
the parent and on this tree alternately (nothing bench.py runs is touched here: the ranges should overlap).

The JSON goes to --out and to stdout.  There is no CPU fallback: without a GPU the tool fails."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_sparse import HBM_BYTES_PER_S, K, M_SYMBOLS, PROB, SEED, T, git_head, spread, timed  # noqa: E402
from bench_sumprod import against_parent  # noqa: E402
from flash_viterbi_amd import decoder, hostio  # noqa: E402
from flash_viterbi_amd.generate_data import data_script  # noqa: E402

NSEQ = 8
FP64_FLOPS_PER_S = 157.3e12 / 2          # the float64 vector rate: half the float32 vector rate


def kernel_stats(path):
    """{short kernel name: times in us} of the fvc:: and fvs:: kernels of a rocprofv3 kernel_stats CSV"""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            for ns in ("fvc::", "fvs::"):
                if ns in name:
                    short = name.split(ns, 1)[1].split("(", 1)[0]
                    out[short] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3,
                                      max_us=float(row["MaxNs"]) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--parent-root", default="", metavar="DIR")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--kernel-stats", default="", metavar="CSV", help="kernel_stats CSV of a --trace-child kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "counts_bench.json"))
    ap.add_argument("--git-head", default="")
    ap.add_argument("--trace-child", action="store_true", help="only a fixed number of calls, for a kernel trace")
    args = ap.parse_args()
    if args.alternations < 5 or args.min_seconds < 0.5:
        print("note: fewer than 5 alternations or less than 0.5 s per timing: not a result to quote", file=sys.stderr)
    A64, B64, Pi64 = data_script.make_model64(K, M_SYMBOLS, SEED, PROB)
    A, B, Pi = hostio.quantize_text16(A64), hostio.quantize_text16(B64), hostio.quantize_text16(Pi64)
    del A64
    ob = np.asarray(data_script.make_observations(T, M_SYMBOLS, SEED), dtype=np.int32)
    obs = [np.ascontiguousarray(np.roll(ob, 7 * s)) for s in range(NSEQ)]
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        if args.trace_child:
            for _ in range(20):
                fv.expected_counts([ob])
            print("trace child done")
            return

        def posteriors_of(seqs):
            total = 0.0
            for o in seqs:
                fv.posteriors(o, want_gamma=False)
                total += fv.sumprod_stats()["gpu_ms"]
            return total

        last = {}
        calls = {}
        for n in (1, NSEQ):
            seqs = obs[:n]
            calls[f"counts_{n}"] = (lambda seqs=seqs: fv.expected_counts(seqs), lambda: fv.counts_stats()["gpu_ms"])
            calls[f"posteriors_{n}"] = (lambda seqs=seqs, n=n: last.__setitem__(n, posteriors_of(seqs)), lambda n=n: last[n])
        facts = {}
        for name, (fn, _) in calls.items():                 # warm (the tables are built here), and what a call counts
            fn()
            if name.startswith("counts"):
                st = fv.counts_stats()
                facts[name] = {k: st[k] for k in ("sequences", "dead_sequences", "times", "step_launches", "task_steps", "xi_launches",
                                                  "wide_times", "device_bytes")}
        ms = {n: [] for n in calls}
        wall = {n: [] for n in calls}
        for _ in range(args.alternations):
            for name, (fn, gpu_ms) in calls.items():
                wall[name].append(1e3 * timed(fn, args.min_seconds))
                ms[name].append(gpu_ms())
        out = dict(tool="tools/bench_counts.py", git_head=git_head(args.git_head), min_seconds=args.min_seconds,
                   alternations=args.alternations, K=K, T=T, M=M_SYMBOLS, batch_sequences=NSEQ,
                   gpu_ms={n: spread(ms[n]) for n in calls}, wall_ms_per_call={n: spread(wall[n]) for n in calls}, calls=facts,
                   xi_byte_floor_us=1e6 * 20.0 * K * K / HBM_BYTES_PER_S,
                   xi_flop_floor_us=1e6 * 2.0 * K * K * (T - 1) / FP64_FLOPS_PER_S, fp64_flops_per_s=FP64_FLOPS_PER_S)
        for n in (1, NSEQ):
            out[f"counts_over_posteriors_{n}"] = out["gpu_ms"][f"counts_{n}"]["median"] / out["gpu_ms"][f"posteriors_{n}"]["median"]
        out["counting_costs_more_than_the_two_passes"] = bool(out["counts_over_posteriors_1"] > 2.0)
        if args.kernel_stats and os.path.isfile(args.kernel_stats):
            out["kernel_trace"] = kernel_stats(args.kernel_stats)
            xi = out["kernel_trace"].get("counts_xi")
            if xi:
                out["xi_kernel_us"] = xi["average_us"]
                out["xi_kernel_over_floor"] = xi["average_us"] / max(out["xi_byte_floor_us"], out["xi_flop_floor_us"])
        else:
            out["kernel_trace"] = "not measured: no --kernel-stats file of a --trace-child kernel trace"
    finally:
        fv.close()
    if args.parent_root:
        out["bench_py_against_parent"] = against_parent(os.path.abspath(args.parent_root), args.alternations, args.bench_steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
