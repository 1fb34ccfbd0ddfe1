#!/usr/bin/env python3
"""bench_emissions.py — decodes from per-time emission scores (fv_set_emissions) against the symbol decode of the same
sequence, and what staging costs.

  python tools/bench_emissions.py [--min-seconds 0.5] [--alternations 5] [--no-kernel-trace]
                                  [--parent-tree DIR [--parent-head REV]]
                                  [--out profiles/emissions_bench.json] [--git-head REV]
  python tools/bench_emissions.py --stage-only N      # N stagings of each form and nothing else (the run to trace)

Shape: bench.py's model (K = 3965, M = 50, density 0.112, seed 12), T = 256, n_split = 8, FV_MODE_REFERENCE (cfg2), under
the library's AUTO kernel, in ONE process on one context.

(a) decodes: variant `symbols` is decode_full(ob); variant `emissions` is decode_full(ob=None) on the table-derived rows
    logE[t][i] = log(B[i][ob[t]]) of the same sequence, staged once.  Paths, scores and step kernels are compared first
    (exactly).  Then the two alternate: each timing is a host clock around repeated calls (every call ends in the
    library's own synchronise) worth at least --min-seconds, --alternations times after a warm-up; per variant the
    median and range of ms per decode, and the ratio of the medians beside the run-to-run range.  Both launch the same
    kernels on the same number of launches: a ratio beyond that range needs an explanation.
(b) staging: fv_set_emissions from host float32, host float64 and device float32 (a block made by the test hook), host
    clock per call (fv_stats.set_emissions_ms of the last call beside it).  The kernel's own time is taken twice:
    device events around 200 back-to-back launches of stage_emissions<TIN> on a device block (the test hook
    fv_test_stage_emissions_ms; five such timings per TIN), beside the floor (sizeof(TIN) + 12) * T * K bytes at 8 TB/s
    plus one launch (3 us); and from a child run of this tool (--stage-only) under `rocprofv3
    --kernel-trace --stats`: mean, min and max per stage_emissions<TIN>, which hold no launch and so stand beside the
    bytes alone.  Where the profiler is missing or fails the entry says "not measured" and why.
(c) the symbol path against the parent commit (--parent-tree DIR: a built checkout of the parent): `bench.py --gpus 1
    --steps 100 --warmup 10` as a child process in DIR and in this tree, alternated three times; ms_per_step of every run
    and whether each tree's median lies inside the other's range.  Without --parent-tree the entry says "not measured".

The JSON goes to --out and to stdout.  There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import csv
import glob
import json
import math
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from flash_viterbi_amd import decoder, hostio  # noqa: E402
from flash_viterbi_amd.generate_data import data_script  # noqa: E402

K, T, M_SYMBOLS, PROB, SEED, N_SPLIT = 3965, 256, 50, 0.112, 12, 8
HBM_BYTES_PER_S, LAUNCH_S = 8e12, 3e-6


def git_head(given):
    if given:
        return given
    try:
        res = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, timeout=30)
        if res.returncode == 0:
            dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, timeout=30).stdout.strip()
            return res.stdout.strip() + ("+modified" if dirty else "")
    except (OSError, subprocess.SubprocessError):
        pass
    return "unknown (not a git checkout; pass --git-head)"


def timed(fn, min_seconds):
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / calls


def spread(values):
    v = sorted(values)
    med = statistics.median(v)
    return dict(median=med, min=v[0], max=v[-1], range_rel=(v[-1] - v[0]) / med if med else 0.0)


def libm_log(x):
    """log of every float32 entry through math.log (the host libm's, what fv_set_model calls); log 0 = -inf"""
    vals, inv = np.unique(np.ascontiguousarray(x, dtype=np.float32).reshape(-1), return_inverse=True)
    table = np.array([math.log(float(v)) if v > 0 else -math.inf for v in vals], dtype=np.float64)
    return table[inv].reshape(x.shape)


def workload():
    A64, B64, Pi64 = data_script.make_model64(K, M_SYMBOLS, SEED, PROB)
    A, B, Pi = hostio.quantize_text16(A64), hostio.quantize_text16(B64), hostio.quantize_text16(Pi64)
    ob = np.asarray(data_script.make_observations(T, M_SYMBOLS, SEED), dtype=np.int32)
    logE = np.ascontiguousarray(libm_log(B)[:, ob].T)          # [T][K]
    return A, B, Pi, ob, logE


def stage_forms(fv, logE):
    """{name: (fn, element bytes)}; the device block lives until the returned release() is called"""
    e32 = np.ascontiguousarray(logE.astype(np.float32))
    ptr = fv.test_device_alloc(e32)
    forms = {"host_f32": (lambda: fv.set_emissions(e32), 4), "host_f64": (lambda: fv.set_emissions(logE), 8),
             "device_f32": (lambda: fv.set_emissions((ptr, np.float32, T, K)), 4)}
    return forms, (lambda: fv.test_device_free(ptr))


def stage_only(n):
    A, B, Pi, ob, logE = workload()
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        forms, release = stage_forms(fv, logE)
        try:
            for fn, _ in forms.values():
                for _ in range(n):
                    fn()
        finally:
            release()
    finally:
        fv.close()


def kernel_trace(n):
    """stage_emissions<TIN> durations out of a child run under rocprofv3, or the reason there are none"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return dict(status="not measured", reason="rocprofv3 not found")
    tmp = tempfile.mkdtemp(prefix="emis_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "stage", "--",
               sys.executable, os.path.abspath(__file__), "--stage-only", str(n)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        except subprocess.TimeoutExpired:
            return dict(status="not measured", reason="the traced child ran beyond 600 s")
        if res.returncode != 0:
            return dict(status="not measured", reason=f"the traced child ended with {res.returncode}", stderr=res.stderr[-600:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return dict(status="not measured", reason="no kernel_stats.csv in the profiler's output")
        out = {}
        with open(files[0], newline="") as fh:
            for row in csv.DictReader(fh):
                if "stage_emissions" in row["Name"]:
                    tin = "f64" if "<double>" in row["Name"] else "f32"
                    bytes_s = ((8 if tin == "f64" else 4) + 12) * T * K / HBM_BYTES_PER_S      # (a trace holds no launch)
                    mean_us = float(row["AverageNs"]) * 1e-3
                    out[f"stage_emissions<{tin}>"] = dict(calls=int(row["Calls"]), mean_us=mean_us, min_us=float(row["MinNs"]) * 1e-3,
                                                          max_us=float(row["MaxNs"]) * 1e-3, bytes_floor_us=1e6 * bytes_s,
                                                          bytes_floor_over_mean=1e6 * bytes_s / mean_us if mean_us else None)
        return dict(status="measured" if out else "not measured", kernels=out, stagings_per_form=n)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def kernel_events(fv, logE, reps=200, timings=5):
    """device events around `reps` back-to-back launches of stage_emissions<TIN> on a device block, `timings` times"""
    out = {}
    for tin, block in (("f32", np.ascontiguousarray(logE.astype(np.float32))), ("f64", np.ascontiguousarray(logE))):
        ptr = fv.test_device_alloc(block)
        try:
            us = [1e3 * fv.test_stage_emissions_ms(ptr, block.dtype, T, K, reps) for _ in range(timings)]
        finally:
            fv.test_device_free(ptr)
        bytes_s = (block.itemsize + 12) * T * K / HBM_BYTES_PER_S
        sp = spread(us)
        out[f"stage_emissions<{tin}>"] = dict(us_per_launch=sp, launches_per_timing=reps, bytes_floor_us=1e6 * bytes_s,
                                              floor_us=1e6 * (bytes_s + LAUNCH_S), floor_over_median=1e6 * (bytes_s + LAUNCH_S) / sp["median"])
    return dict(status="measured", kernels=out)


def bench_step_ms(tree):
    """ms_per_step of one `bench.py --gpus 1 --steps 100 --warmup 10` run as a child process in `tree`"""
    res = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "100", "--warmup", "10"], cwd=tree,
                         capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} ended with {res.returncode}:\n{res.stderr[-1500:]}")
    for line in reversed(res.stdout.splitlines()):
        if line.startswith("{"):
            return float(json.loads(line)["ms_per_step"])
    raise RuntimeError(f"bench.py in {tree} printed no result line")


def symbol_path_against_parent(parent_tree, parent_head, rounds=3):
    if not parent_tree:
        return dict(status="not measured", reason="no --parent-tree")
    ms = {"parent": [], "this": []}
    for _ in range(rounds):
        ms["parent"].append(bench_step_ms(os.path.abspath(parent_tree)))
        ms["this"].append(bench_step_ms(ROOT))
    sp = {n: spread(v) for n, v in ms.items()}
    inside = all(sp[b]["min"] <= sp[a]["median"] <= sp[b]["max"] for a, b in (("this", "parent"), ("parent", "this")))
    print(f"bench.py ms_per_step: parent {ms['parent']}, this {ms['this']}", file=sys.stderr, flush=True)
    return dict(status="measured", command="bench.py --gpus 1 --steps 100 --warmup 10", parent_head=parent_head or "not given",
                ms_per_step_in_run_order=ms, parent=sp["parent"], this=sp["this"],
                this_over_parent_median=sp["this"]["median"] / sp["parent"]["median"], each_median_inside_the_others_range=inside)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--no-kernel-trace", action="store_true")
    ap.add_argument("--stage-only", type=int, default=0, metavar="N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emissions_bench.json"))
    ap.add_argument("--git-head", default="")
    ap.add_argument("--parent-tree", default="", metavar="DIR", help="a built checkout of the parent commit, for (c)")
    ap.add_argument("--parent-head", default="", metavar="REV")
    args = ap.parse_args()
    if args.stage_only:
        stage_only(args.stage_only)
        return
    if args.alternations < 5 or args.min_seconds < 0.5:
        print("note: fewer than 5 alternations or less than 0.5 s per timing: not a result to quote", file=sys.stderr)
    out = dict(tool="tools/bench_emissions.py", git_head=git_head(args.git_head), min_seconds=args.min_seconds,
               alternations=args.alternations, hbm_bytes_per_s=HBM_BYTES_PER_S, launch_s=LAUNCH_S,
               K=K, T=T, M=M_SYMBOLS, density=PROB, seed=SEED, n_split=N_SPLIT, mode="reference")
    A, B, Pi, ob, logE = workload()
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        out["set_model_ms"] = fv.stats()["set_model_ms"]
        fv.set_emissions(logE)
        run = {"symbols": lambda: fv.decode_full(ob, N_SPLIT), "emissions": lambda: fv.decode_full(None, N_SPLIT, T=T)}
        facts = {}
        for _ in range(3):                                      # warm both, compare exactly
            res = {}
            for name, fn in run.items():
                res[name] = fn()
                st = fv.stats()
                facts[name] = dict(kernel=st["kernel"], step_launches=st["step_launches"], task_steps=st["task_steps"], passes=st["passes"])
            a, b = res["symbols"], res["emissions"]
            assert a[2] == b[2] == 0 and a[0].tolist() == b[0].tolist() and a[1] == b[1], "the emission decode differs from the symbol decode"
            assert facts["symbols"] == facts["emissions"], "the two decodes launched differently"
        ms = {n: [] for n in run}
        gpu_ms = {n: [] for n in run}
        for _ in range(args.alternations):
            for name, fn in run.items():
                ms[name].append(1e3 * timed(fn, args.min_seconds))
                gpu_ms[name].append(fv.stats()["gpu_ms"])
        dec = {n: dict(ms_per_decode=spread(ms[n]), gpu_ms_last_call=spread(gpu_ms[n]), **facts[n]) for n in run}
        rng = max(dec[n]["ms_per_decode"]["range_rel"] for n in run)
        ratio = dec["emissions"]["ms_per_decode"]["median"] / dec["symbols"]["ms_per_decode"]["median"]
        out["decodes"] = dict(variants=dec, paths_equal=True, emissions_over_symbols_median=ratio, run_to_run_range_rel=rng,
                              ratio_within_range=abs(ratio - 1.0) <= rng)
        print(f"decode: symbols {dec['symbols']['ms_per_decode']['median']:.3f} ms, emissions {dec['emissions']['ms_per_decode']['median']:.3f} ms: "
              f"x{ratio:.4f} (run-to-run range {rng:.4f})", file=sys.stderr, flush=True)
        forms, release = stage_forms(fv, logE)
        try:
            staging = {}
            for name, (fn, esz) in forms.items():
                fn()
                per = [1e3 * timed(fn, args.min_seconds) for _ in range(3)]
                staging[name] = dict(ms_per_call=spread(per), set_emissions_ms_last_call=fv.stats()["set_emissions_ms"],
                                     input_bytes=esz * T * K, table_bytes=12 * T * K)
            out["staging"] = staging
        finally:
            release()
        out["stage_kernel_events"] = kernel_events(fv, logE)
        out["device_bytes_with_tables"] = fv.stats()["device_bytes"]
    finally:
        fv.close()
    out["symbol_path_against_parent"] = symbol_path_against_parent(args.parent_tree, args.parent_head)
    out["stage_kernel_trace"] = (dict(status="not measured", reason="--no-kernel-trace") if args.no_kernel_trace else kernel_trace(20))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
