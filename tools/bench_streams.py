#!/usr/bin/env python3
"""bench_streams.py — fv_streams_*, many online streams on one context, beside the only way there was before it: one
context with one fv_stream per sequence, pushed round-robin.  One process; the two arms are alternated,
at least --min-seconds each, --alternations times; medians and ranges.

  python tools/bench_streams.py [--models cfg2,cfg2_u16,large] [--slots 1,4,8,16,32] [--pushes 16,64]
                                [--min-seconds 0.5] [--alternations 5] [--large-k 262144] [--kernel-trace MODEL]
                                [--out profiles/streams_bench.json] [--git-head REV]
  python tools/bench_streams.py --trace-child set|contexts --kernel-trace MODEL    # 8 slots, pushes of 64, nothing else (the run to trace)

Models: cfg2 (bench.py's model, K = 3965, set dense) on the library default kernel and under FV_KERNEL_U16_REFINE, and
the CSR-set model of K = 262144 (--large-k) of tools/bench_stream.py.  Every sequence has T = 256 times; slot s decodes
the observations rotated by 37 * s.  Per model, number of slots S and push length:
  set           arm A: one context, fv_streams_open(S), every call pushes the next times of all S slots
  contexts      arm B: S contexts with one fv_stream each, the same pushes round-robin
The figure is wall time per consumed time, summed over the slots (S * T times per run), of the push calls alone: opens
and closes are outside the clock.  Beside it stands the part of that time the library counted inside its calls
(push_ms_total): the difference is the Python wrapper, which packs S sequences per call for the set.  ratio_contexts_over_set > 1: the set is faster.  Both arms' pieces are compared with
the one-shot path first.  device_bytes: what the device holds more than before the arm's contexts were made (the model
tables and the open streams), from hipMemGetInfo.
--kernel-trace MODEL adds the kernel times of both arms on that model, S = 8, pushes of 64, each from a child run of this tool under
`rocprofv3 --kernel-trace --stats`.  A result for a model is merged into the JSON at --out, which keeps the others.
There is no CPU fallback: without a GPU the tool fails."""
import argparse
import csv
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_sparse import K, M_SYMBOLS, PROB, SEED, git_head, spread  # noqa: E402
from flash_viterbi_amd import decoder, hostio  # noqa: E402
from flash_viterbi_amd.generate_data import data_script  # noqa: E402

D = decoder
T = 256


def device_used():
    """bytes in use on the device (total - free), or None where the runtime library cannot be asked"""
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            hip = ctypes.CDLL(name)
        except OSError:
            continue
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0:
            return total.value - free.value
    return None


class Model:
    def __init__(self, name, large_k):
        self.name = name
        if name == "large":
            self.csr = data_script.make_model_csr(large_k, M_SYMBOLS, SEED, 32)
            self.ob = np.random.RandomState(SEED).randint(0, M_SYMBOLS, T).astype(np.int32)
            self.facts = dict(K=large_k, M=M_SYMBOLS, mean_in_degree=float(self.csr[0][-1]) / large_k, seed=SEED,
                              model="CSR-set, FV_KERNEL_AUTO")
        else:
            A64, B64, Pi64 = data_script.make_model64(K, M_SYMBOLS, SEED, PROB)
            self.dense = tuple(hostio.quantize_text16(x) for x in (A64, B64, Pi64))
            self.ob = np.asarray(data_script.make_observations(T, M_SYMBOLS, SEED), dtype=np.int32)
            self.facts = dict(K=K, M=M_SYMBOLS, density=PROB, seed=SEED,
                              model="dense-set, " + ("FV_KERNEL_U16_REFINE" if name == "cfg2_u16" else "FV_KERNEL_AUTO"))

    def context(self):
        fv = decoder.FlashViterbi(0)
        if self.name == "large":
            fv.set_model_sparse(*self.csr)
        else:
            fv.set_model(*self.dense)
            if self.name == "cfg2_u16":
                fv.set_option(D.OPT_KERNEL, D.KERNEL_U16_REFINE)
        return fv

    def seq(self, s):
        return np.ascontiguousarray(np.roll(self.ob, 37 * s))


def run_set(fv, obs, push):
    """arm A: one run; returns (seconds in the push calls, path per slot, seconds the library counted inside them)"""
    S = len(obs)
    ids = list(range(S))
    fv.streams_open(S)
    pieces = [[] for _ in ids]
    spent = 0.0
    for pos in range(0, T, push):
        chunk = [o[pos:pos + push] for o in obs]
        t0 = time.perf_counter()
        got, _ = fv.streams_push(ids, obs=chunk)
        spent += time.perf_counter() - t0
        for s in ids:
            pieces[s].append(got[s])
    for s in ids:
        pieces[s].append(fv.streams_close(s)[0])
    inside = 1e-3 * fv.streams_stats()["push_ms_total"]
    fv.streams_end()
    return spent, [np.concatenate(p) for p in pieces], inside


def run_contexts(ctxs, obs, push):
    """arm B: one run; returns (seconds in the push calls, path per sequence, seconds the library counted inside them)"""
    for fv in ctxs:
        fv.stream_open()
    pieces = [[] for _ in ctxs]
    spent = 0.0
    for pos in range(0, T, push):
        chunk = [o[pos:pos + push] for o in obs]
        t0 = time.perf_counter()
        for fv, c, p in zip(ctxs, chunk, pieces):
            p.append(fv.stream_push(ob=c))
        spent += time.perf_counter() - t0
    inside = 0.0
    for fv, p in zip(ctxs, pieces):
        p.append(fv.stream_close()[0])
        inside += 1e-3 * fv.stream_stats()["push_ms_total"]
    return spent, [np.concatenate(p) for p in pieces], inside


def timed_us_per_time(run, S, min_seconds):
    """runs until min_seconds have passed; microseconds per consumed time of the push calls, and of the library inside them
    (fv_streams_stats / fv_stream_stats push_ms_total: the calls without the Python wrapper)"""
    spent, inside, runs, t0 = 0.0, 0.0, 0, time.perf_counter()
    while time.perf_counter() - t0 < min_seconds:
        got = run()
        spent += got[0]
        inside += got[2]
        runs += 1
    return 1e6 * spent / (runs * S * T), 1e6 * inside / (runs * S * T)


def measure(model, slots, pushes, args):
    out = dict(T=T, **model.facts)
    set_fv = model.context()
    after_set_ctx = device_used()
    ctxs = [model.context() for _ in range(max(slots))]
    after_ctxs = device_used()
    try:
        out["kernel"] = None
        want = {}
        for S in slots:
            obs = [model.seq(s) for s in range(S)]
            for s in range(S):
                if s not in want:
                    res = ctxs[0].decode_full(obs[s], 1, D.MODE_SINGLE_PASS)
                    assert res[2] == 0
                    want[s] = res[0].tolist()
            # device memory with the streams open: one context and a set of S, against S contexts with a stream each
            mem = None
            if after_ctxs is not None:
                set_fv.streams_open(S)
                with_set = device_used()
                set_fv.streams_end()
                for fv in ctxs[:S]:
                    fv.stream_open()
                with_streams = device_used()
                for fv in ctxs[:S]:
                    fv.stream_abort()
                per_ctx = (after_ctxs - after_set_ctx) // len(ctxs)
                mem = dict(set=per_ctx + (with_set - after_ctxs),
                           contexts=S * per_ctx + (with_streams - after_ctxs))
                mem["ratio_contexts_over_set"] = mem["contexts"] / mem["set"] if mem["set"] else None
            for push in pushes:
                arms = dict(set=lambda: run_set(set_fv, obs, push), contexts=lambda: run_contexts(ctxs[:S], obs, push))
                for name, run in arms.items():                   # warm, and compare exactly
                    paths = run()[1]
                    assert [p.tolist() for p in paths] == [want[s] for s in range(S)], f"{model.name} S={S} push={push}: {name} differs from the one-shot path"
                st = set_fv.streams_stats()
                out["kernel"] = st["kernel"]
                wall, lib = dict(set=[], contexts=[]), dict(set=[], contexts=[])
                for _ in range(args.alternations):
                    for name, run in arms.items():
                        w, inside = timed_us_per_time(run, S, args.min_seconds)
                        wall[name].append(w)
                        lib[name].append(inside)
                a, b = spread(wall["set"]), spread(wall["contexts"])
                ratios = sorted(y / x for x, y in zip(wall["set"], wall["contexts"]))
                out[f"S{S}_push{push}"] = dict(
                    slots=S, push=push, set_us_per_time=a, contexts_us_per_time=b,
                    set_us_per_time_inside_the_library=spread(lib["set"]),
                    contexts_us_per_time_inside_the_library=spread(lib["contexts"]),
                    ratio_contexts_over_set=dict(of_medians=b["median"] / a["median"], min=ratios[0], max=ratios[-1]),
                    set_counters=dict(batch_cap=st["batch_cap"], calls=st["calls"], step_launches=st["step_launches"],
                                      task_steps=st["task_steps"], check_launches=st["check_launches"],
                                      check_slots=st["check_slots"], syncs=st["syncs"]),
                    device_bytes=mem if mem is not None else "not measured")
                print(f"{model.name} S={S} push={push}: set {a['median']:.2f} us/time, contexts {b['median']:.2f}", file=sys.stderr, flush=True)
    finally:
        for fv in [set_fv] + ctxs:
            fv.close()
    return out


TRACE_RUNS = 10


def trace_child(arm, name, large_k):
    model = Model(name, large_k)
    obs = [model.seq(s) for s in range(8)]
    ctxs = [model.context() for _ in range(1 if arm == "set" else 8)]
    try:
        for _ in range(TRACE_RUNS):
            if arm == "set":
                run_set(ctxs[0], obs, 64)
            else:
                run_contexts(ctxs, obs, 64)
    finally:
        for fv in ctxs:
            fv.close()


def kernel_trace(name, large_k):
    """kernel times of both arms (model `name`, S = 8, pushes of 64) out of child runs under rocprofv3"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return dict(status="not measured", reason="rocprofv3 not found")
    out = {}
    for arm in ("set", "contexts"):
        tmp = tempfile.mkdtemp(prefix="streams_trace_")
        try:
            cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "streams", "--",
                   sys.executable, os.path.abspath(__file__), "--trace-child", arm, "--kernel-trace", name, "--large-k", str(large_k)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired:
                return dict(status="not measured", reason="a traced child ran beyond 300 s", arms=out)
            files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if res.returncode != 0 or not files:
                return dict(status="not measured", reason=f"traced child: exit {res.returncode}, {len(files)} stats files",
                            stderr=res.stderr[-600:], arms=out)
            rows = []
            with open(files[0], newline="") as fh:
                for row in csv.DictReader(fh):
                    rows.append(dict(name=row["Name"][:70], calls=int(row["Calls"]), total_us=float(row["TotalDurationNs"]) * 1e-3,
                                     mean_us=float(row["AverageNs"]) * 1e-3))
            rows.sort(key=lambda r: -r["total_us"])
            out[arm] = dict(kernels=rows[:8], kernel_us_per_time=sum(r["total_us"] for r in rows) / (TRACE_RUNS * 8 * T))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return dict(status="measured", workload=f"{name}, 8 slots, pushes of 64, {TRACE_RUNS} runs per arm (model set-up, open and close included)", arms=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", default="cfg2,cfg2_u16,large")
    ap.add_argument("--slots", default="1,4,8,16,32")
    ap.add_argument("--pushes", default="16,64")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--large-k", type=int, default=262144)
    ap.add_argument("--kernel-trace", default="", metavar="MODEL", help="trace both arms on this model (S = 8, pushes of 64)")
    ap.add_argument("--trace-child", default="", metavar="ARM")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams_bench.json"))
    ap.add_argument("--git-head", default="")
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.trace_child, args.kernel_trace or "cfg2", args.large_k)
        return
    if args.alternations < 5 or args.min_seconds < 0.5:
        print("note: fewer than 5 alternations or less than 0.5 s per timing: not a result to quote", file=sys.stderr)
    slots = [int(x) for x in args.slots.split(",") if x]
    pushes = [int(x) for x in args.pushes.split(",") if x]
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            out = json.load(fh)
    out.update(tool="tools/bench_streams.py", git_head=git_head(args.git_head), min_seconds=args.min_seconds,
               alternations=args.alternations)
    for name in [m for m in args.models.split(",") if m]:
        out[name] = measure(Model(name, args.large_k), slots, pushes, args)
    if args.kernel_trace:
        out["kernel_trace_" + args.kernel_trace] = kernel_trace(args.kernel_trace, args.large_k)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
