#!/usr/bin/env python3
"""bench_sparse_beam.py — FLASH-BS on models set through fv_set_model_sparse (FV_OPT_SPARSE_BEAM): the CSR scatter + finish
step against the dense row gather on the same model, a model no dense table can hold, and the dense path against another
build of the library.

  python tools/bench_sparse_beam.py [--min-seconds 0.5] [--alternations 5] [--skip-large] [--large-k 262144]
                                    [--only-large] [--parent-tree DIR] [--out profiles/sparse_beam_bench.json] [--git-head REV]

(a) The same model set dense and set sparse under the option, in ONE process on two contexts, T = 256, n_split = 8,
    FV_MODE_REFERENCE: bench.py's cfg2 model (K = 3965, M = 50, density 0.112, seed 12) at B = 32 and B = 256, and K = 16384
    (the same distributions from data_script.make_model32_fast: generating cfg4's own model takes minutes) at B = 256.
    Paths, scores and return codes are compared first (exactly).  Then the two decodes alternate: each timing is a host
    clock around repeated fv_decode_beam calls worth at least --min-seconds, --alternations times; per variant the median
    and the range of ms per decode, the event time of the whole-sequence pass, and the decode's statistics.
(b) K = 262144 (--large-k) with about 32 edges per state (data_script.make_model_csr, never a dense array), T = 256,
    n_split = 8, B = 1024, sparse only: same protocol.  --only-large runs nothing else (for a kernel trace of this case).
(c) --parent-tree DIR: a built checkout of the commit to compare the DENSE path with.  `bench.py --gpus 1 --workload cfg4`
    and the flash_bs entry of `bench.py --gpus 1 --workload cfg2 --full --no-cpu-baseline` run alternately from this tree
    and from DIR, --alternations times each; medians and ranges of both.  The dense medians of this tree must lie inside
    the other tree's own run-to-run range (recorded as inside_parent_range).

The JSON goes to --out and to stdout.  There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from flash_viterbi_amd import decoder, hostio  # noqa: E402
from flash_viterbi_amd.generate_data import data_script  # noqa: E402

T, M_SYMBOLS, PROB, SEED, N_SPLIT = 256, 50, 0.112, 12, 8
STAT_KEYS = ("kernel", "table_bytes_per_step", "device_bytes", "step_launches", "task_steps", "passes", "beam_exact_sets", "beam_ties",
             "beam_spec_steps", "beam_reach_events", "beam_cand_selects", "beam_list_short", "beam_list_long")


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
    return dict(median=med, min=v[0], max=v[-1], range_rel=(v[-1] - v[0]) / med if med else 0.0, runs=len(v))


def alternate(variants, min_seconds, alternations):
    """variants: {name: (fn, fv)}.  Per name: ms per decode and the event time of the whole-sequence pass, over the alternations."""
    ms = {n: [] for n in variants}
    top = {n: [] for n in variants}
    for _ in range(alternations):
        for name, (fn, fv) in variants.items():
            ms[name].append(1e3 * timed(fn, min_seconds))
            top[name].append(fv.stats()["top_pass_ms"])
    out = {}
    for name, (fn, fv) in variants.items():
        st = fv.stats()
        out[name] = dict(ms_per_decode=spread(ms[name]), top_pass_ms=spread(top[name]), gpu_ms_last=st["gpu_ms"],
                         stats={k: st[k] for k in STAT_KEYS})
    return out


def same(a, b):
    return a[2] == b[2] and a[0].tolist() == b[0].tolist() and np.float32(a[1]).view(np.uint32) == np.float32(b[1]).view(np.uint32)


def part_pair(args, K, beams):
    if K == 3965:
        A64, B64, Pi64 = data_script.make_model64(K, M_SYMBOLS, SEED, PROB)
        A, B, Pi = hostio.quantize_text16(A64), hostio.quantize_text16(B64), hostio.quantize_text16(Pi64)
        del A64
    else:
        A, B, Pi = data_script.make_model32_fast(K, M_SYMBOLS, SEED, PROB)
    ob = np.asarray(data_script.make_observations(T, M_SYMBOLS, SEED), dtype=np.int32)
    nnz = int(np.count_nonzero(A))
    dense, sparse = decoder.FlashViterbi(0), decoder.FlashViterbi(0)
    out = []
    try:
        dense.set_model(A, B, Pi)
        sparse.set_model_sparse(*decoder.dense_to_csr(A), B, Pi)
        sparse.set_option(decoder.OPT_SPARSE_BEAM, 1)
        del A
        for beam in beams:
            run = {"dense_set": (lambda: dense.decode_beam(ob, N_SPLIT, beam), dense),
                   "sparse_set": (lambda: sparse.decode_beam(ob, N_SPLIT, beam), sparse)}
            for _ in range(2):                                    # warm both, compare exactly
                assert same(run["dense_set"][0](), run["sparse_set"][0]()), "sparse-set beam decode differs from dense-set"
            assert sparse.stats()["kernel"] == decoder.KERNEL_CSR_F64
            res = alternate(run, args.min_seconds, args.alternations)
            d, s = res["dense_set"]["ms_per_decode"], res["sparse_set"]["ms_per_decode"]
            out.append(dict(K=K, T=T, M=M_SYMBOLS, density=PROB, seed=SEED, n_split=N_SPLIT, beam=beam, mode="reference", stored_entries=nnz,
                            variants=res, sparse_over_dense_median=s["median"] / d["median"],
                            run_to_run_range_rel=max(d["range_rel"], s["range_rel"])))
            print(f"K={K} B={beam}: dense-set {d['median']:.3f} ms, sparse-set {s['median']:.3f} ms per decode "
                  f"(x{s['median'] / d['median']:.2f})", file=sys.stderr, flush=True)
    finally:
        dense.close()
        sparse.close()
    return out


def part_large(args):
    k, beam = args.large_k, 1024
    t0 = time.perf_counter()
    ip, ix, dt, B, Pi = data_script.make_model_csr(k, M_SYMBOLS, SEED, 32)
    gen_s = time.perf_counter() - t0
    ob = np.random.RandomState(SEED).randint(0, M_SYMBOLS, T).astype(np.int32)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model_sparse(ip, ix, dt, B, Pi)
        fv.set_option(decoder.OPT_SPARSE_BEAM, 1)
        set_ms = fv.stats()["set_model_ms"]
        fn = lambda: fv.decode_beam(ob, N_SPLIT, beam)            # noqa: E731
        first = fn()
        assert same(first, fn())
        res = alternate({"sparse_set": (fn, fv)}, args.min_seconds, args.alternations)["sparse_set"]
        steps = T - 1
        res.update(K=k, T=T, M=M_SYMBOLS, beam=beam, n_split=N_SPLIT, mode="reference", seed=SEED, stored_entries=int(ip[-1]),
                   mean_out_degree=float(ip[-1]) / k, generator_s=gen_s, set_model_ms=set_ms, return_code=int(first[2]),
                   dense_tables_fv_set_model_would_need_bytes=16 * k * k,
                   top_pass_lockstep_us_median=1e3 * res["top_pass_ms"]["median"] / steps,
                   entries_scattered_per_step_estimate=beam * float(ip[-1]) / k, cells_a_dense_step_would_touch=beam * k)
        print(f"K={k} B={beam}: {res['ms_per_decode']['median']:.2f} ms per decode, {res['top_pass_lockstep_us_median']:.1f} us per lock-step "
              f"of the whole-sequence pass", file=sys.stderr, flush=True)
        return res
    finally:
        fv.close()


def bench_line(tree, extra):
    res = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1"] + extra, cwd=tree, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"bench.py failed in {tree}:\n{res.stdout[-2000:]}{res.stderr[-2000:]}")
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def part_parent(args):
    trees = {"this": ROOT, "parent": os.path.abspath(args.parent_tree)}
    cases = {"cfg4_ms_per_decode": (["--workload", "cfg4", "--steps", "10", "--warmup", "2"], lambda j: j["decode_ms"]),
             "cfg2_full_flash_bs_decode_ms": (["--workload", "cfg2", "--steps", "20", "--warmup", "3", "--full", "--no-cpu-baseline"],
                                              lambda j: j["flash_bs"]["decode_ms"])}
    out = {}
    for name, (extra, pick) in cases.items():
        vals = {t: [] for t in trees}
        raw = {}
        for _ in range(args.alternations):
            for t, tree in trees.items():
                j = bench_line(tree, extra)
                raw[t] = {k: j.get(k) for k in ("metric", "unit", "value")}
                vals[t].append(float(pick(j)))
        s = {t: spread(v) for t, v in vals.items()}
        out[name] = dict(bench_args=extra, reported=raw, this=s["this"], parent=s["parent"],
                         inside_parent_range=s["parent"]["min"] <= s["this"]["median"] <= s["parent"]["max"],
                         this_over_parent_median=s["this"]["median"] / s["parent"]["median"])
        print(f"{name}: this {s['this']['median']:.4g} [{s['this']['min']:.4g}, {s['this']['max']:.4g}]  parent {s['parent']['median']:.4g} "
              f"[{s['parent']['min']:.4g}, {s['parent']['max']:.4g}]", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--only-large", action="store_true")
    ap.add_argument("--large-k", type=int, default=262144)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_beam_bench.json"))
    ap.add_argument("--git-head", default="")
    args = ap.parse_args()
    if args.alternations < 5 or args.min_seconds < 0.5:
        print("note: fewer than 5 alternations or less than 0.5 s per timing: not a result to quote", file=sys.stderr)
    out = dict(tool="tools/bench_sparse_beam.py", git_head=git_head(args.git_head), min_seconds=args.min_seconds, alternations=args.alternations)
    if not args.only_large:
        out["same_model_dense_and_sparse"] = part_pair(args, 3965, (32, 256)) + part_pair(args, 16384, (256,))
    if not args.skip_large:
        out["large"] = part_large(args)
    if args.parent_tree and not args.only_large:
        out["dense_path_against_parent"] = part_parent(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
