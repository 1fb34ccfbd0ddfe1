#!/usr/bin/env python3
"""bench_stream.py — fv_stream_*, the online full-state decode, beside the one-shot single-pass decode of the same
sequence on the same box.  One process; a stream run and a one-shot decode are alternated, at least
--min-seconds each, --alternations times; medians and ranges.

  python tools/bench_stream.py [--min-seconds 0.5] [--alternations 5] [--skip-large] [--large-k 262144]
                               [--no-kernel-trace] [--parent-step-us cfg2=..,cfg3=..,large=..]
                               [--out profiles/stream_bench.json] [--git-head REV]
  python tools/bench_stream.py --trace-child CE     # cfg2 in pushes of 64 at check_every = CE and nothing else (the run to trace)

Workloads: cfg2 (bench.py's model, K = 3965, T = 256), cfg3 (the same model, T = 4096), both set dense under the default
kernel, and a CSR-set model of K = 262144 (--large-k) with about 32 in-edges per state, T = 256.  Per workload:
  one_shot      top_steps_ms / (T - 1) of fv_decode_full(ob, T, 1, FV_MODE_SINGLE_PASS): device events around the T - 1 step
                launches, and the wall time of the call per time.  --parent-step-us records beside it the same figure
                taken from the parent commit's library by the same tool code (that path is not touched by the stream).
  stream        pushes of 16 / 64 / 256 symbols at the default check interval: wall time per time, open, pushes and
                close included (every push ends in a synchronise), the ratio to the one-shot wall time per time, both also
                net of open_close_us_per_stream (an empty stream opened and closed: the buffers allocated, cleared and
                freed, paid once per stream whatever its length), mean lag over the pushes, largest lag, arg rows
                allocated; the pieces are compared with the one-shot path first.
  check_every   pushes of 64 at check_every = 1, 4, 8, 16, 32, 64: wall time per time, checks, commits, mean and largest
                lag.  The default interval is chosen on these at cfg2.
  per_push      pushes of 1: wall time per push (one step, one check, the synchronise, and on a commit the back-track and
                the copy), beside the time per time of one push of T (one synchronise in all): the fixed cost of a push.
Kernel times of stream_ancestors / stream_verdict by check_every come from a child run of this tool (--trace-child)
under `rocprofv3 --kernel-trace --stats` (cfg2, pushes of 64).

The JSON goes to --out and to stdout.  There is no CPU fallback: without a GPU the tool fails."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_sparse import K, M_SYMBOLS, PROB, SEED, git_head, spread, timed  # noqa: E402
from flash_viterbi_amd import decoder, hostio  # noqa: E402
from flash_viterbi_amd.generate_data import data_script  # noqa: E402

D = decoder
INTERVALS = (1, 4, 8, 16, 32, 64)


def dense_context():
    A64, B64, Pi64 = data_script.make_model64(K, M_SYMBOLS, SEED, PROB)
    fv = decoder.FlashViterbi(0)
    fv.set_model(hostio.quantize_text16(A64), hostio.quantize_text16(B64), hostio.quantize_text16(Pi64))
    return fv


def stream_once(fv, ob, push, check_every):
    """one stream over ob in pushes of `push`; returns (path, score, rc, lags after every push)"""
    fv.stream_open(0, check_every)
    pieces, lags = [], []
    for pos in range(0, ob.size, push):
        pieces.append(fv.stream_push(ob=ob[pos:pos + push]))
        lags.append(fv.stream_pending())
    last, score, rc = fv.stream_close()
    return np.concatenate(pieces + [last]), score, rc, lags


def measure(fv, ob, args, pushes=(16, 64, 256)):
    T = ob.size
    one = lambda: fv.decode_full(ob, 1, D.MODE_SINGLE_PASS)      # noqa: E731
    ref = one()
    assert ref[2] == 0
    variants = {("stream", p, 0): (lambda p=p: stream_once(fv, ob, p, 0)) for p in pushes}
    variants.update({("check_every", 64, ce): (lambda ce=ce: stream_once(fv, ob, 64, ce)) for ce in INTERVALS})
    variants[("per_push", 1, 0)] = lambda: stream_once(fv, ob[:min(T, 512)], 1, 0)
    variants[("per_push", T, 0)] = lambda: stream_once(fv, ob, T, 0)
    facts = {}
    for key, fn in variants.items():                             # warm, compare exactly, note what the run counts
        got = fn()
        n = got[0].size
        assert got[2] == 0 and (n < T or (got[0].tolist() == ref[0].tolist() and got[1] == ref[1])), f"{key}: stream differs from the one-shot decode"
        assert n == T or got[0].tolist() == one_prefix(fv, ob[:n]), key
        st = fv.stream_stats()
        facts[key] = dict(times=n, pushes=st["pushes"], checks=st["checks"], commits=st["commits"], lag_max=st["lag_max"],
                          lag_mean=float(np.mean(got[3])), arg_rows_capacity=st["arg_rows_capacity"], regrows=st["regrows"],
                          kernel=st["kernel"])
    def open_close():
        fv.stream_open(0, 0)
        fv.stream_close()
    wall = {key: [] for key in variants}
    shot_wall, shot_step, per_stream = [], [], []
    for _ in range(args.alternations):
        shot_wall.append(1e6 * timed(one, args.min_seconds) / T)
        per_stream.append(1e6 * timed(open_close, min(args.min_seconds, 0.2)))
        shot_step.append(1e3 * fv.stats()["top_steps_ms"] / (T - 1))
        for key, fn in variants.items():
            wall[key].append(1e6 * timed(fn, args.min_seconds) / facts[key]["times"])
    out = dict(T=T, kernel=fv.stats()["kernel"],
               one_shot=dict(step_us_device_events=spread(shot_step), wall_us_per_time=spread(shot_wall)))
    shot = out["one_shot"]["wall_us_per_time"]["median"]
    out["open_close_us_per_stream"] = spread(per_stream)        # an empty stream: the buffers allocated, cleared and freed
    oc = out["open_close_us_per_stream"]["median"]
    for group in ("stream", "check_every", "per_push"):
        out[group] = {}
        for key in variants:
            if key[0] != group:
                continue
            name = f"push_{key[1]}" if group != "check_every" else f"check_every_{key[2]}"
            w = spread(wall[key])
            net = w["median"] - oc / facts[key]["times"]
            out[group][name] = dict(wall_us_per_time=w, ratio_to_one_shot_wall=w["median"] / shot,
                                    wall_us_per_time_net_of_open_close=net, ratio_net_of_open_close=net / shot, **facts[key])
    p1, pT = out["per_push"]["push_1"], out["per_push"][f"push_{T}"]
    out["per_push"]["fixed_cost_us_per_push"] = p1["wall_us_per_time"]["median"] - pT["wall_us_per_time"]["median"]
    return out


def one_prefix(fv, ob):
    """the one-shot path of a prefix (the per-push run of a long sequence streams only its head)"""
    return fv.decode_full(ob, 1, D.MODE_SINGLE_PASS)[0].tolist()


def trace_child(ce):
    fv = dense_context()
    try:
        ob = np.asarray(data_script.make_observations(256, M_SYMBOLS, SEED), dtype=np.int32)
        for _ in range(20):
            stream_once(fv, ob, 64, ce)
    finally:
        fv.close()


def kernel_trace():
    """stream_ancestors / stream_verdict durations by check_every out of child runs under rocprofv3"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return dict(status="not measured", reason="rocprofv3 not found")
    out = {}
    for ce in INTERVALS:
        tmp = tempfile.mkdtemp(prefix="stream_trace_")
        try:
            cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "stream", "--",
                   sys.executable, os.path.abspath(__file__), "--trace-child", str(ce)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired:
                return dict(status="not measured", reason="a traced child ran beyond 300 s", by_check_every=out)
            files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if res.returncode != 0 or not files:
                return dict(status="not measured", reason=f"traced child: exit {res.returncode}, {len(files)} stats files",
                            stderr=res.stderr[-600:], by_check_every=out)
            rows = {}
            with open(files[0], newline="") as fh:
                for row in csv.DictReader(fh):
                    for name in ("stream_ancestors", "stream_verdict"):
                        if name in row["Name"]:
                            rows[name] = dict(calls=int(row["Calls"]), mean_us=float(row["AverageNs"]) * 1e-3,
                                              min_us=float(row["MinNs"]) * 1e-3, max_us=float(row["MaxNs"]) * 1e-3)
                    if "trellis_step" in row["Name"]:
                        rows.setdefault("step_kernels", []).append(dict(name=row["Name"][:60], calls=int(row["Calls"]),
                                                                        mean_us=float(row["AverageNs"]) * 1e-3))
            out[f"check_every_{ce}"] = rows
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return dict(status="measured", workload="cfg2, pushes of 64, 20 streams", by_check_every=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--large-k", type=int, default=262144)
    ap.add_argument("--no-kernel-trace", action="store_true")
    ap.add_argument("--parent-step-us", default="", help="cfg2=..,cfg3=..,large=..: the one-shot step time on the parent commit")
    ap.add_argument("--one-shot-only", action="store_true", help="only the one-shot figures (runs on a library without fv_stream_*)")
    ap.add_argument("--trace-child", type=int, default=0, metavar="CE")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.json"))
    ap.add_argument("--git-head", default="")
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.trace_child)
        return
    if args.alternations < 5 or args.min_seconds < 0.5:
        print("note: fewer than 5 alternations or less than 0.5 s per timing: not a result to quote", file=sys.stderr)
    parent = {k: float(v) for k, v in (kv.split("=") for kv in args.parent_step_us.split(",") if kv)}
    out = dict(tool="tools/bench_stream.py", git_head=git_head(args.git_head), min_seconds=args.min_seconds,
               alternations=args.alternations)

    def one_shot_only(fv, ob):
        one = lambda: fv.decode_full(ob, 1, D.MODE_SINGLE_PASS)      # noqa: E731
        one()
        steps = []
        for _ in range(args.alternations):
            timed(one, args.min_seconds)
            steps.append(1e3 * fv.stats()["top_steps_ms"] / (ob.size - 1))
        return dict(T=int(ob.size), one_shot=dict(step_us_device_events=spread(steps)))

    run = one_shot_only if args.one_shot_only else (lambda fv, ob: measure(fv, ob, args))
    fv = dense_context()
    try:
        for name, T in (("cfg2", 256), ("cfg3", 4096)):
            ob = np.asarray(data_script.make_observations(T, M_SYMBOLS, SEED), dtype=np.int32)
            out[name] = dict(K=K, M=M_SYMBOLS, density=PROB, seed=SEED, model="dense-set, FV_KERNEL_AUTO", **run(fv, ob))
            print(f"{name}: done", file=sys.stderr, flush=True)
    finally:
        fv.close()
    if not args.skip_large:
        ip, ix, dt, B, Pi = data_script.make_model_csr(args.large_k, M_SYMBOLS, SEED, 32)
        ob = np.random.RandomState(SEED).randint(0, M_SYMBOLS, 256).astype(np.int32)
        fv = decoder.FlashViterbi(0)
        try:
            fv.set_model_sparse(ip, ix, dt, B, Pi)
            out["large"] = dict(K=args.large_k, M=M_SYMBOLS, mean_in_degree=float(ip[-1]) / args.large_k, seed=SEED,
                                model="CSR-set, FV_KERNEL_AUTO", **run(fv, ob))
        finally:
            fv.close()
    for name, us in parent.items():
        if name in out:
            out[name]["one_shot"]["step_us_device_events_parent_commit"] = us
    if not args.no_kernel_trace and not args.one_shot_only:
        out["kernel_trace"] = kernel_trace()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
