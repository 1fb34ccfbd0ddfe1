#!/usr/bin/env python3
"""bench_sumprod.py — fv_loglik, fv_loglik_batch and fv_posteriors on the cfg2 model (K = 3965, T = 256) beside their
yardstick on the same box.  One process; the measured calls are alternated, at least --min-seconds each,
--alternations times; medians and ranges.

  python tools/bench_sumprod.py [--min-seconds 0.5] [--alternations 5] [--parent-root DIR] [--bench-steps 20]
                                [--out profiles/sumprod_bench.json] [--git-head REV]

What it records, per alternation from the HIP-event time of the call (fv_sumprod_stats.gpu_ms, fv_stats.top_steps_ms):
  loglik_step_us             fv_loglik: event time / its T - 1 step launches (init, table check and final log-sum included)
  loglik_batch_task_step_us  fv_loglik_batch of 32 sequences of T = 256: event time / task steps
  posteriors_step_us         fv_posteriors: event time / its 2 (T - 1) step launches (the gamma kernel included)
  yardstick_step_us          fv_decode_full(..., 1, FV_MODE_SINGLE_PASS) under FV_KERNEL_F32_REFINE: the whole-sequence
                             pass's step launches alone (top_steps_ms / (T - 1)); it streams the same 4 B per cell
and the wall time per call of each, the ratio loglik_step_us / yardstick_step_us (target 1.25), the byte floor
4 K^2 / 8 TB/s.
--parent-root: a built checkout of the parent commit.  `python bench.py --gpus 1 --steps N` is then run in child processes
on the parent and on this tree alternately, and both sets of values are recorded: nothing bench.py runs is touched here, so
the medians should lie within each other's run-to-run range.

  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sumprod.py --trace-child
runs 20 fv_loglik, 20 fv_posteriors and 5 fv_loglik_batch calls and nothing else: the kernel times of profiles/sumprod_kernel_stats.csv.

The JSON goes to --out and to stdout.  There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_sparse import HBM_BYTES_PER_S, K, M_SYMBOLS, PROB, SEED, T, git_head, spread, timed  # noqa: E402
from flash_viterbi_amd import decoder, hostio  # noqa: E402
from flash_viterbi_amd.generate_data import data_script  # noqa: E402

NSEQ = 32


def bench_child(root, steps):
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3"],
                         capture_output=True, text=True, timeout=900, cwd=root)
    if res.returncode != 0:
        raise RuntimeError(f"bench.py in {root}: exit {res.returncode}\n{res.stderr[-600:]}")
    return json.loads(res.stdout.strip().splitlines()[-1])


def against_parent(parent_root, alternations, steps):
    runs = {"parent": [], "this": []}
    try:
        for _ in range(alternations):
            for who, root in (("parent", parent_root), ("this", ROOT)):
                runs[who].append(bench_child(root, steps))
    except (RuntimeError, subprocess.SubprocessError, ValueError) as e:
        return dict(status="not measured", reason=str(e)[-800:])
    p, t = spread([r["value"] for r in runs["parent"]]), spread([r["value"] for r in runs["this"]])
    return dict(status="measured", command=f"python bench.py --gpus 1 --steps {steps} --warmup 3", alternations=alternations,
                metric=runs["this"][0].get("metric"), unit=runs["this"][0].get("unit"), parent=p, this=t, ratio=t["median"] / p["median"],
                within_run_to_run_range=bool(t["min"] <= p["max"] and p["min"] <= t["max"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--parent-root", default="", metavar="DIR")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sumprod_bench.json"))
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
    fv, yard = decoder.FlashViterbi(0), decoder.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        yard.set_model(A, B, Pi)
        yard.set_option(decoder.OPT_KERNEL, decoder.KERNEL_F32_REFINE)

        if args.trace_child:
            for _ in range(20):
                fv.loglik(ob)
                fv.posteriors(ob, want_gamma=False)
            for _ in range(5):
                fv.loglik_batch(obs)
            print("trace child done")
            return

        def sumprod_us(per):
            st = fv.sumprod_stats()
            return 1e3 * st["gpu_ms"] / st[per]

        calls = {
            "loglik": (lambda: fv.loglik(ob), lambda: sumprod_us("step_launches")),
            "loglik_batch": (lambda: fv.loglik_batch(obs), lambda: sumprod_us("task_steps")),
            "posteriors": (lambda: fv.posteriors(ob, want_gamma=False), lambda: sumprod_us("step_launches")),
            "yardstick": (lambda: yard.decode_full(ob, 1, decoder.MODE_SINGLE_PASS), lambda: 1e3 * yard.stats()["top_steps_ms"] / (T - 1)),
        }
        facts = {}
        for name, (fn, _) in calls.items():                 # warm (the tables are built here), and what a call counts
            fn()
            if name != "yardstick":
                st = fv.sumprod_stats()
                facts[name] = {k: st[k] for k in ("step_launches", "task_steps", "passes", "batch_cap", "table_bytes_per_step",
                                                  "device_bytes", "refine_columns", "refine_finite")}
            else:
                facts[name] = dict(kernel=yard.stats()["kernel"], table_bytes_per_step=yard.stats()["table_bytes_per_step"])
        us = {n: [] for n in calls}
        wall = {n: [] for n in calls}
        for _ in range(args.alternations):
            for name, (fn, per_step) in calls.items():
                wall[name].append(1e3 * timed(fn, args.min_seconds))
                us[name].append(per_step())
        out = dict(tool="tools/bench_sumprod.py", git_head=git_head(args.git_head), min_seconds=args.min_seconds,
                   alternations=args.alternations, K=K, T=T, M=M_SYMBOLS, batch_sequences=NSEQ,
                   byte_floor_step_us=1e6 * 4.0 * K * K / HBM_BYTES_PER_S,
                   loglik_step_us=spread(us["loglik"]), loglik_batch_task_step_us=spread(us["loglik_batch"]),
                   posteriors_step_us=spread(us["posteriors"]), yardstick_step_us=spread(us["yardstick"]),
                   wall_ms_per_call={n: spread(wall[n]) for n in calls}, calls=facts, target_ratio=1.25)
        out["loglik_step_over_yardstick"] = out["loglik_step_us"]["median"] / out["yardstick_step_us"]["median"]
        out["posteriors_step_over_yardstick"] = out["posteriors_step_us"]["median"] / out["yardstick_step_us"]["median"]
        out["target_met"] = bool(out["loglik_step_over_yardstick"] <= 1.25)
    finally:
        fv.close()
        yard.close()
    if args.parent_root:
        out["bench_py_against_parent"] = against_parent(os.path.abspath(args.parent_root), args.alternations, args.bench_steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
