#!/usr/bin/env python3
"""bench_sparse_f64.py — FV_KERNEL_CSR_F64, the float64 walk over a CSR-set model (trellis_step_csr_f64), against the only
route a model with entries above 1 had before it (set dense, FV_KERNEL_F64_STREAM), against the filter walk on a model both
can take, and on a model fv_set_model cannot hold.  Protocol of tools/bench_sparse.py: one process, alternating variants
of at least --min-seconds each, --alternations times, median and range.

  python tools/bench_sparse_f64.py [--min-seconds 0.5] [--alternations 5] [--skip-large] [--large-k 262144]
                                   [--out profiles/sparse_f64_bench.json] [--git-head REV]

(a) cfg2: bench.py's model (K = 3965, M = 50, density 0.112, seed 12), T = 256, n_split = 8, FV_MODE_REFERENCE.
    "above_one": 1 % of its stored entries replaced by values in (1, 50]; the model set dense under FV_KERNEL_F64_STREAM
    (the yardstick: 8 * nrows * K bytes of table per step) against the model set through fv_set_model_sparse under
    FV_KERNEL_CSR_F64 (12 bytes per padded entry).  Paths and scores are compared first (exactly).
    "unit_range": the unscaled model set through fv_set_model_sparse, FV_KERNEL_AUTO (the filter walk, 6 bytes per padded
    entry) against FV_KERNEL_CSR_F64, for orientation.
(b) K = 262144 (--large-k) with about 32 in-edges per state (data_script.make_model_csr), T = 256, n_split = 8, under
    FV_KERNEL_CSR_F64, with the filter walk beside it.

The JSON goes to --out and to stdout.  There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_sparse import K, M_SYMBOLS, N_SPLIT, PROB, SEED, T, alternate, git_head, model_facts, profiled  # noqa: E402
from flash_viterbi_amd import decoder, hostio  # noqa: E402
from flash_viterbi_amd.generate_data import data_script  # noqa: E402

D = decoder


def above_one(data, frac, seed):
    rs = np.random.RandomState(seed)
    out = np.array(data, dtype=np.float32, copy=True)
    pick = np.nonzero(rs.uniform(size=out.size) < frac)[0]
    out[pick] = np.maximum(rs.uniform(1.0, 50.0, pick.size).astype(np.float32), np.nextafter(np.float32(1), np.float32(2)))
    return out, int(pick.size)


def compare(variants, names, args, nnz):
    """Warm both, compare exactly, alternate; returns the per-variant results and the ratio second / first."""
    a, b = (variants[n] for n in names)
    for _ in range(3):
        ra, rb = a[0](), b[0]()
        assert ra[2] == rb[2] == 0 and ra[0].tolist() == rb[0].tolist() and ra[1] == rb[1], f"{names[1]} differs from {names[0]}"
    res = alternate({n: variants[n] for n in names}, args.min_seconds, args.alternations)
    for n in names:
        fn, fv, _ = variants[n]
        fn()
        res[n].update(model_facts(fv, nnz))
        res[n]["profiled"] = profiled(fv, fn)
    first, second = res[names[0]], res[names[1]]
    return dict(variants=res,
                decode_ratio_median=second["ms_per_decode"]["median"] / first["ms_per_decode"]["median"],
                step_ratio_median=second["top_pass_step_us"]["median"] / first["top_pass_step_us"]["median"],
                streamed_bytes_ratio=second["table_bytes_per_step"] / float(first["table_bytes_per_step"]),
                run_to_run_range_rel=max(first["ms_per_decode"]["range_rel"], second["ms_per_decode"]["range_rel"]))


def part_cfg2(args):
    A64, B64, Pi64 = data_script.make_model64(K, M_SYMBOLS, SEED, PROB)
    A, B, Pi = hostio.quantize_text16(A64), hostio.quantize_text16(B64), hostio.quantize_text16(Pi64)
    del A64
    ob = np.asarray(data_script.make_observations(T, M_SYMBOLS, SEED), dtype=np.int32)
    ip, ix, dt = decoder.dense_to_csr(A)
    nnz = int(ip[-1])
    big, nbig = above_one(dt, 0.01, SEED)
    Abig = A.copy()
    Abig[np.repeat(np.arange(K), np.diff(ip)), ix] = big
    dense, sparse, unit = decoder.FlashViterbi(0), decoder.FlashViterbi(0), decoder.FlashViterbi(0)
    try:
        dense.set_model(Abig, B, Pi)
        dense.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM)
        sparse.set_model_sparse(ip, ix, big, B, Pi)
        sparse.set_option(D.OPT_KERNEL, D.KERNEL_CSR_F64)
        out = dict(K=K, T=T, M=M_SYMBOLS, density=PROB, seed=SEED, n_split=N_SPLIT, mode="reference", stored_entries=nnz,
                   entries_above_one=nbig)
        run = {"dense_set_f64_stream": (lambda: dense.decode_full(ob, N_SPLIT), dense, T - 1),
               "sparse_set_csr_f64": (lambda: sparse.decode_full(ob, N_SPLIT), sparse, T - 1)}
        out["above_one"] = compare(run, ("dense_set_f64_stream", "sparse_set_csr_f64"), args, nnz)
        st = out["above_one"]["variants"]
        assert st["dense_set_f64_stream"]["kernel"] == D.KERNEL_F64_STREAM and st["sparse_set_csr_f64"]["kernel"] == D.KERNEL_CSR_F64

        def under(kernel):
            def fn():
                unit.set_option(D.OPT_KERNEL, kernel)
                return unit.decode_full(ob, N_SPLIT)
            return fn
        unit.set_model_sparse(ip, ix, dt, B, Pi)
        run = {"sparse_set_filter_walk": (under(D.KERNEL_AUTO), unit, T - 1), "sparse_set_csr_f64": (under(D.KERNEL_CSR_F64), unit, T - 1)}
        out["unit_range"] = compare(run, ("sparse_set_filter_walk", "sparse_set_csr_f64"), args, nnz)
        st = out["unit_range"]["variants"]
        assert st["sparse_set_filter_walk"]["kernel"] == D.KERNEL_SPARSE_CSR and st["sparse_set_csr_f64"]["kernel"] == D.KERNEL_CSR_F64
        return out
    finally:
        dense.close()
        sparse.close()
        unit.close()


def part_large(args):
    k = args.large_k
    t0 = time.perf_counter()
    ip, ix, dt, B, Pi = data_script.make_model_csr(k, M_SYMBOLS, SEED, 32)
    gen_s = time.perf_counter() - t0
    ob = np.random.RandomState(SEED).randint(0, M_SYMBOLS, T).astype(np.int32)
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model_sparse(ip, ix, dt, B, Pi)

        def under(kernel):
            def fn():
                fv.set_option(D.OPT_KERNEL, kernel)
                return fv.decode_full(ob, N_SPLIT)
            return fn
        run = {"sparse_set_filter_walk": (under(D.KERNEL_AUTO), fv, T - 1), "sparse_set_csr_f64": (under(D.KERNEL_CSR_F64), fv, T - 1)}
        out = dict(K=k, T=T, M=M_SYMBOLS, mean_in_degree=float(ip[-1]) / k, seed=SEED, n_split=N_SPLIT, mode="reference",
                   generator_s=gen_s, dense_table_bytes_fv_set_model_would_need=8 * k * k)
        out.update(compare(run, ("sparse_set_filter_walk", "sparse_set_csr_f64"), args, int(ip[-1])))
        v = out["variants"]["sparse_set_csr_f64"]
        step_s = 1e-6 * v["top_pass_step_us"]["median"]
        out["csr_f64_step_streamed_bytes_per_s"] = v["table_bytes_per_step"] / step_s
        return out
    finally:
        fv.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--large-k", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_f64_bench.json"))
    ap.add_argument("--git-head", default="")
    args = ap.parse_args()
    if args.alternations < 5 or args.min_seconds < 0.5:
        print("note: fewer than 5 alternations or less than 0.5 s per timing: not a result to quote", file=sys.stderr)
    out = dict(tool="tools/bench_sparse_f64.py", git_head=git_head(args.git_head), min_seconds=args.min_seconds,
               alternations=args.alternations)
    out["cfg2"] = part_cfg2(args)
    for part in ("above_one", "unit_range"):
        c = out["cfg2"][part]
        names = list(c["variants"])
        print(f"cfg2 {part}: {names[0]} {c['variants'][names[0]]['ms_per_decode']['median']:.3f} ms, {names[1]} "
              f"{c['variants'][names[1]]['ms_per_decode']['median']:.3f} ms per decode: x{c['decode_ratio_median']:.3f} "
              f"(streamed bytes x{c['streamed_bytes_ratio']:.3f}, spread {c['run_to_run_range_rel']:.3f})", file=sys.stderr, flush=True)
    if not args.skip_large:
        out["large"] = part_large(args)
        g = out["large"]
        print(f"K={g['K']}: filter walk {g['variants']['sparse_set_filter_walk']['ms_per_decode']['median']:.2f} ms, float64 walk "
              f"{g['variants']['sparse_set_csr_f64']['ms_per_decode']['median']:.2f} ms per decode; float64 walk "
              f"{g['variants']['sparse_set_csr_f64']['top_pass_step_us']['median']:.1f} us per step, "
              f"{g['csr_f64_step_streamed_bytes_per_s'] / 1e12:.2f} TB/s streamed", file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
