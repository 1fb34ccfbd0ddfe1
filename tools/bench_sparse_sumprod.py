#!/usr/bin/env python3
"""bench_sparse_sumprod.py — fv_loglik / fv_loglik_batch / fv_posteriors on models set by fv_set_model_sparse under
fv_set_sparse_sumprod, beside their yardsticks on the same box.  One process; the measured calls are
alternated, at least --min-seconds each, --alternations times; medians and ranges.

  python tools/bench_sparse_sumprod.py [--min-seconds 0.5] [--alternations 5] [--skip-large] [--large-k 262144]
                                       [--kernel-stats CSV] [--parent-root DIR] [--bench-steps 20]
                                       [--out profiles/sparse_sumprod_bench.json] [--git-head REV]

Per alternation, from the HIP-event time of the call (fv_sumprod_stats.gpu_ms: first to last kernel, so the scale launches of
the memory form, the init rows and the final sum are inside) divided by its step launches (task steps for the batch):
(a) cfg2 (K = 3965, density 0.112, T = 256), the same model set three ways: by fv_set_model (the dense route of this
    commit), by fv_set_model_sparse with the score rows staged in LDS, and by fv_set_model_sparse with FV_OPT_DEBUG bit 31
    (score rows left in memory by the scale launch).  fv_loglik and fv_posteriors us per step, the ratios, which CSR form is
    the faster one.
(b) K = 262144 (--large-k), about 32 edges per state (data_script.make_model_csr drawn over the whole K, no blocks), T = 64:
    fv_loglik us per step, fv_posteriors us per step over both passes and its backward pass alone (the call's event time
    minus the median of fv_loglik's, per step), fv_loglik_batch of 8 per task step, and the yardstick
    fv_decode_full(ob, 1, FV_MODE_SINGLE_PASS) under FV_KERNEL_CSR_F64 on the same context (top_steps_ms / (T - 1)).
--kernel-stats: the kernel_stats CSV of a `rocprofv3 --kernel-trace --stats -- python tools/bench_sparse_sumprod.py
    --trace-child large` run (or `cfg2`); the average time of every sumprod_* kernel is copied into the JSON, and the scale
    launch's time per step is the sum of sumprod_rowmax's and sumprod_scale's.  Without it that figure is marked unmeasured.
--parent-root: a built checkout of the parent commit; `python bench.py --gpus 1 --steps N --warmup 3` is run in child
    processes on the parent and on this tree alternately and both ranges are recorded.

The JSON goes to --out and to stdout.  There is no CPU fallback: without a GPU the tool fails."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_sparse import K, M_SYMBOLS, PROB, SEED, T, git_head, spread, timed  # noqa: E402
from bench_sumprod import bench_child  # noqa: E402
from flash_viterbi_amd import decoder, hostio  # noqa: E402
from flash_viterbi_amd.generate_data import data_script  # noqa: E402

D = decoder
LARGE_T, LARGE_NSEQ = 64, 8
FACTS = ("step_launches", "task_steps", "passes", "batch_cap", "table_bytes_per_step", "device_bytes", "refine_columns", "refine_finite")


def step_us(fv, per="step_launches"):
    st = fv.sumprod_stats()
    return 1e3 * st["gpu_ms"] / st[per]


def measure(calls, args):
    """calls: {name: (fn, per_step)}.  Warm each once (tables are built there), then alternate."""
    facts = {}
    for name, (fn, _, fv) in calls.items():
        fn()
        if fv is not None:
            st = fv.sumprod_stats()
            facts[name] = {k: st[k] for k in FACTS}
            facts[name]["forms"] = hex(fv.test_sumprod_forms())
    us = {n: [] for n in calls}
    wall = {n: [] for n in calls}
    for _ in range(args.alternations):
        for name, (fn, per_step, _) in calls.items():
            wall[name].append(1e3 * timed(fn, args.min_seconds))
            us[name].append(per_step())
    return ({n: spread(v) for n, v in us.items()}, {n: spread(v) for n, v in wall.items()}, facts)


def cfg2_contexts():
    A64, B64, Pi64 = data_script.make_model64(K, M_SYMBOLS, SEED, PROB)
    A, B, Pi = hostio.quantize_text16(A64), hostio.quantize_text16(B64), hostio.quantize_text16(Pi64)
    del A64
    ob = np.asarray(data_script.make_observations(T, M_SYMBOLS, SEED), dtype=np.int32)
    ctxs = dict(dense=D.FlashViterbi(0), csr_lds=D.FlashViterbi(0), csr_mem=D.FlashViterbi(0))
    ctxs["dense"].set_model(A, B, Pi)
    csr = D.dense_to_csr(A)
    for n in ("csr_lds", "csr_mem"):
        ctxs[n].set_model_sparse(*csr, B, Pi)
        ctxs[n].set_sparse_sumprod(1)
    ctxs["csr_mem"].set_option(D.OPT_DEBUG, D.DEBUG_CSR_ROWS_IN_MEMORY)
    return ctxs, ob, int(csr[0][-1])


def part_cfg2(args):
    ctxs, ob, nnz = cfg2_contexts()
    try:
        calls = {}
        for n, fv in ctxs.items():
            calls[n + "_loglik"] = (lambda fv=fv: fv.loglik(ob), lambda fv=fv: step_us(fv), fv)
            calls[n + "_posteriors"] = (lambda fv=fv: fv.posteriors(ob, want_gamma=False), lambda fv=fv: step_us(fv), fv)
        lls = [ctxs[n].loglik(ob) for n in ctxs]
        assert lls[1] == lls[2] and abs(lls[0] - lls[1]) <= 1e-9 * abs(lls[0]), lls
        us, wall, facts = measure(calls, args)
        out = dict(K=K, T=T, M=M_SYMBOLS, density=PROB, seed=SEED, stored_entries=nnz, step_us=us, wall_ms_per_call=wall, calls=facts)
        for call in ("loglik", "posteriors"):
            lds, mem, dense = (us[f"{n}_{call}"]["median"] for n in ("csr_lds", "csr_mem", "dense"))
            out[call + "_csr_lds_over_dense"] = lds / dense
            out[call + "_csr_mem_over_dense"] = mem / dense
            out[call + "_faster_csr_form"] = "lds" if lds < mem else "mem"
        return out
    finally:
        for fv in ctxs.values():
            fv.close()


def large_context(k):
    t0 = time.perf_counter()
    ip, ix, dt, B, Pi = data_script.make_model_csr(k, M_SYMBOLS, SEED, 32)
    gen_s = time.perf_counter() - t0
    ob = np.random.RandomState(SEED).randint(0, M_SYMBOLS, LARGE_T).astype(np.int32)
    fv = D.FlashViterbi(0)
    fv.set_model_sparse(ip, ix, dt, B, Pi)
    fv.set_sparse_sumprod(1)
    fv.set_option(D.OPT_KERNEL, D.KERNEL_CSR_F64)
    return fv, ob, int(ip[-1]), gen_s


def part_large(args):
    fv, ob, nnz, gen_s = large_context(args.large_k)
    try:
        obs = [np.ascontiguousarray(np.roll(ob, 7 * s)) for s in range(LARGE_NSEQ)]
        calls = {
            "loglik": (lambda: fv.loglik(ob), lambda: step_us(fv), fv),
            "posteriors": (lambda: fv.posteriors(ob, want_gamma=False), lambda: step_us(fv), fv),
            "loglik_batch": (lambda: fv.loglik_batch(obs), lambda: step_us(fv, "task_steps"), fv),
            "yardstick": (lambda: fv.decode_full(ob, 1, D.MODE_SINGLE_PASS), lambda: 1e3 * fv.stats()["top_steps_ms"] / (LARGE_T - 1), None),
        }
        us, wall, facts = measure(calls, args)
        assert fv.stats()["kernel"] == D.KERNEL_CSR_F64
        out = dict(K=args.large_k, T=LARGE_T, M=M_SYMBOLS, mean_out_degree=nnz / float(args.large_k), stored_entries=nnz, seed=SEED,
                   batch_sequences=LARGE_NSEQ, generator_s=gen_s, step_us=us, wall_ms_per_call=wall, calls=facts,
                   yardstick="fv_decode_full(ob, 1, FV_MODE_SINGLE_PASS) under FV_KERNEL_CSR_F64, top_steps_ms / (T - 1)",
                   yardstick_table_bytes_per_step=fv.stats()["table_bytes_per_step"])
        # the backward pass alone: a posteriors call is fv_loglik's launches, T - 1 backward steps, the backward init row and the path kernel
        ll_ms = 1e-3 * us["loglik"]["median"] * (LARGE_T - 1)
        post_ms = 1e-3 * us["posteriors"]["median"] * 2 * (LARGE_T - 1)
        out["posteriors_backward_step_us_derived"] = 1e3 * (post_ms - ll_ms) / (LARGE_T - 1)
        out["loglik_step_over_yardstick"] = us["loglik"]["median"] / us["yardstick"]["median"]
        out["run_to_run_range_rel"] = max(us["loglik"]["range_rel"], us["yardstick"]["range_rel"])
        out["no_slower_than_yardstick"] = bool(us["loglik"]["min"] <= us["yardstick"]["max"])
        out["loglik_streamed_bytes_per_s"] = facts["loglik"]["table_bytes_per_step"] / (1e-6 * us["loglik"]["median"])
        return out
    finally:
        fv.close()


def trace_child(which, large_k):
    """a fixed number of calls and nothing else, for a kernel trace"""
    if which == "large":
        fv, ob, _, _ = large_context(large_k)
        ctxs = {"large": fv}
    else:
        ctxs, ob, _ = cfg2_contexts()
        ctxs.pop("dense").close()
    try:
        for fv in ctxs.values():
            for _ in range(10):
                fv.loglik(ob)
                fv.posteriors(ob, want_gamma=False)
    finally:
        for fv in ctxs.values():
            fv.close()
    print("trace child done")


def kernel_stats(path):
    """{short kernel name: AverageNs / 1000} of the sumprod_* kernels of a rocprofv3 kernel_stats CSV"""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            if "fvs::sumprod_" not in name:
                continue
            short = name.split("fvs::", 1)[1].split("(", 1)[0]
            out[short] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3,
                              max_us=float(row["MaxNs"]) / 1e3)
    scale = [out[k]["average_us"] for k in ("sumprod_rowmax", "sumprod_scale") if k in out]
    return dict(status="measured", source=os.path.basename(path), kernels=out,
                scale_launch_us_per_step=sum(scale) if len(scale) == 2 else None)


def against_parent(parent_root, alternations, steps):
    """bench.py in child processes, the parent commit's checkout and this tree alternately"""
    runs = {"parent": [], "this": []}
    try:
        for i in range(alternations):
            for who, root in (("parent", parent_root), ("this", ROOT)):
                runs[who].append(bench_child(root, steps))
                print(f"bench.py {who} {i + 1}/{alternations}: {runs[who][-1]['value']:.4g}", file=sys.stderr, flush=True)
    except (RuntimeError, OSError, ValueError) as e:
        return dict(status="not measured", reason=str(e)[-800:])
    p, t = spread([r["value"] for r in runs["parent"]]), spread([r["value"] for r in runs["this"]])
    return dict(status="measured", command=f"python bench.py --gpus 1 --steps {steps} --warmup 3", alternations=alternations,
                metric=runs["this"][0].get("metric"), unit=runs["this"][0].get("unit"), parent=p, this=t, ratio=t["median"] / p["median"],
                ranges_overlap=bool(t["min"] <= p["max"] and p["min"] <= t["max"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--skip-cfg2", action="store_true")
    ap.add_argument("--large-k", type=int, default=262144)
    ap.add_argument("--kernel-stats", default="", metavar="CSV")
    ap.add_argument("--parent-root", default="", metavar="DIR")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_sumprod_bench.json"))
    ap.add_argument("--git-head", default="")
    ap.add_argument("--trace-child", choices=("cfg2", "large"), default="")
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args.trace_child, args.large_k)
        return
    if args.alternations < 5 or args.min_seconds < 0.5:
        print("note: fewer than 5 alternations or less than 0.5 s per timing: not a result to quote", file=sys.stderr)
    out = dict(tool="tools/bench_sparse_sumprod.py", git_head=git_head(args.git_head), min_seconds=args.min_seconds,
               alternations=args.alternations)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():                                   # after every part: a later part that fails loses nothing
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    out["cfg2"] = dict(status="not measured", reason="--skip-cfg2") if args.skip_cfg2 else part_cfg2(args)
    save()
    print("cfg2 done", file=sys.stderr, flush=True)
    out["large"] = dict(status="not measured", reason="--skip-large") if args.skip_large else part_large(args)
    save()
    print("large done", file=sys.stderr, flush=True)
    if args.kernel_stats and os.path.isfile(args.kernel_stats):
        out["large_kernel_trace"] = kernel_stats(args.kernel_stats)
    else:
        out["large_kernel_trace"] = dict(status="not measured", reason="no --kernel-stats file: the scale launch's time per step is unmeasured")
    save()
    out["bench_py_against_parent"] = (against_parent(os.path.abspath(args.parent_root), args.alternations, args.bench_steps)
                                      if args.parent_root else dict(status="not measured", reason="no --parent-root"))
    save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
