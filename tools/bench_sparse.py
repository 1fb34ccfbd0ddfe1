#!/usr/bin/env python3
"""bench_sparse.py — models set through fv_set_model_sparse: the walk over a CSR-set model against the parent's sparse walk
over the same model set dense, and a model fv_set_model cannot hold.

  python tools/bench_sparse.py [--min-seconds 0.5] [--alternations 5] [--skip-large] [--large-k 262144]
                               [--out profiles/sparse_model_bench.json] [--git-head REV]

(a) cfg2: bench.py's model (K = 3965, M = 50, density 0.112, seed 12), T = 256, n_split = 8, FV_MODE_REFERENCE, in ONE
    process on two contexts: set dense with FV_KERNEL_SPARSE_Q16 (trellis_step_sparse, the yardstick) and set through
    fv_set_model_sparse (trellis_step_csr).  Paths and scores are compared first (exactly).  Then the two decodes
    alternate: each timing is a host clock around repeated fv_decode_full calls (every call ends in the library's own
    synchronise) worth at least --min-seconds, --alternations times; reported per variant: median and range of ms per
    decode.  The per-step kernel time is the event time around the T - 1 back-to-back step launches of the
    whole-sequence pass (fv_stats.top_steps_ms / (T - 1)), median over the timed decodes' last calls, and — from one
    extra decode under FV_OPT_PROFILE — the mean event time per step launch of the whole decode.
(b) K = 262144 (--large-k) with about 32 in-edges per state (data_script.make_model_csr, never a dense array), T = 256,
    n_split = 8: one decode, and one fv_decode_full_batch of 8 distinct sequences, same protocol.  Achieved bytes per
    second = bytes one step launch streams / per-step kernel time; the step's floor = streamed bytes / 8 TB/s + 3 us
    (a launch of an empty grid).

Every entry carries bytes per stored entry, bytes streamed per step, set_model_ms and device_bytes.  The JSON goes to
--out and to stdout.  There is no CPU fallback: without a GPU the tool fails.
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


def alternate(variants, min_seconds, alternations):
    """variants: {name: (fn, fv)}; fn runs one decode.  Returns per name the ms per decode and the per-step kernel time of
    the whole-sequence pass, over the alternations."""
    ms = {n: [] for n in variants}
    step_us = {n: [] for n in variants}
    for _ in range(alternations):
        for name, (fn, fv, steps) in variants.items():
            ms[name].append(1e3 * timed(fn, min_seconds))
            step_us[name].append(1e3 * fv.stats()["top_steps_ms"] / steps)
    return {n: dict(ms_per_decode=spread(ms[n]), top_pass_step_us=spread(step_us[n])) for n in variants}


def profiled(fv, fn):
    """mean event time per step launch of one decode under FV_OPT_PROFILE (single-stream launches)"""
    fv.set_option(decoder.OPT_PROFILE, 1)
    try:
        fn()
        st = fv.stats()
    finally:
        fv.set_option(decoder.OPT_PROFILE, 0)
    return dict(step_kernel_ms=st["step_kernel_ms"], step_launches=st["step_launches"], task_steps=st["task_steps"],
                mean_launch_us=1e3 * st["step_kernel_ms"] / max(st["step_launches"], 1))


def model_facts(fv, nnz):
    st = fv.stats()
    return dict(kernel=st["kernel"], table_bytes_per_step=st["table_bytes_per_step"], device_bytes=st["device_bytes"],
                set_model_ms=st["set_model_ms"], density=st["density"], stored_entries=int(nnz),
                streamed_bytes_per_stored_entry=st["table_bytes_per_step"] / float(nnz))


def part_cfg2(args):
    A64, B64, Pi64 = data_script.make_model64(K, M_SYMBOLS, SEED, PROB)
    A, B, Pi = hostio.quantize_text16(A64), hostio.quantize_text16(B64), hostio.quantize_text16(Pi64)
    del A64
    ob = np.asarray(data_script.make_observations(T, M_SYMBOLS, SEED), dtype=np.int32)
    nnz = np.count_nonzero(A)
    dense, sparse = decoder.FlashViterbi(0), decoder.FlashViterbi(0)
    try:
        dense.set_model(A, B, Pi)
        dense.set_option(decoder.OPT_KERNEL, decoder.KERNEL_SPARSE_Q16)
        t0 = time.perf_counter()
        csr = decoder.dense_to_csr(A)
        csr_ms = 1e3 * (time.perf_counter() - t0)
        sparse.set_model_sparse(*csr, B, Pi)
        set_ms = {"dense": dense.stats()["set_model_ms"], "sparse": sparse.stats()["set_model_ms"]}
        run = {"dense_set_sparse_q16": (lambda: dense.decode_full(ob, N_SPLIT), dense, T - 1),
               "sparse_set_csr": (lambda: sparse.decode_full(ob, N_SPLIT), sparse, T - 1)}
        for _ in range(3):                                    # warm both, compare exactly
            a, b = dense.decode_full(ob, N_SPLIT), sparse.decode_full(ob, N_SPLIT)
            assert a[2] == b[2] == 0 and a[0].tolist() == b[0].tolist() and a[1] == b[1], "sparse-set decode differs from dense-set"
        assert dense.stats()["kernel"] == decoder.KERNEL_SPARSE_Q16 and sparse.stats()["kernel"] == decoder.KERNEL_SPARSE_CSR
        res = alternate(run, args.min_seconds, args.alternations)
        for name, (fn, fv, _) in run.items():
            res[name].update(model_facts(fv, nnz))
            res[name]["profiled"] = profiled(fv, fn)
        res["dense_set_sparse_q16"]["set_model_ms"] = set_ms["dense"]
        res["sparse_set_csr"]["set_model_ms"] = set_ms["sparse"]
        d, s = res["dense_set_sparse_q16"], res["sparse_set_csr"]
        out = dict(K=K, T=T, M=M_SYMBOLS, density=PROB, seed=SEED, n_split=N_SPLIT, mode="reference", dense_to_csr_ms=csr_ms, variants=res,
                   decode_ratio_median=s["ms_per_decode"]["median"] / d["ms_per_decode"]["median"],
                   step_ratio_median=s["top_pass_step_us"]["median"] / d["top_pass_step_us"]["median"],
                   streamed_bytes_ratio=s["table_bytes_per_step"] / float(d["table_bytes_per_step"]),
                   run_to_run_range_rel=max(d["ms_per_decode"]["range_rel"], s["ms_per_decode"]["range_rel"]))
        out["within_bytes_ratio_plus_spread"] = out["decode_ratio_median"] <= out["streamed_bytes_ratio"] + out["run_to_run_range_rel"]
        return out
    finally:
        dense.close()
        sparse.close()


def part_large(args):
    k = args.large_k
    t0 = time.perf_counter()
    ip, ix, dt, B, Pi = data_script.make_model_csr(k, M_SYMBOLS, SEED, 32)
    gen_s = time.perf_counter() - t0
    rs = np.random.RandomState(SEED)
    obs = [rs.randint(0, M_SYMBOLS, T).astype(np.int32) for _ in range(8)]
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model_sparse(ip, ix, dt, B, Pi)
        set_ms = fv.stats()["set_model_ms"]
        single = lambda: fv.decode_full(obs[0], N_SPLIT)          # noqa: E731
        batch = lambda: fv.decode_full_batch(obs, N_SPLIT)        # noqa: E731
        for _ in range(2):
            p, s, rc = single()
            paths, scores, statuses = batch()
            assert rc == 0 and not statuses.any() and paths[0].tolist() == p.tolist() and scores[0] == s
        res = {}
        for name, fn, nseq in (("single", single, 1), ("batch8", batch, 8)):
            ms, step_us = [], []
            for _ in range(args.alternations):
                ms.append(1e3 * timed(fn, args.min_seconds))
                step_us.append(1e3 * fv.stats()["top_steps_ms"] / (T - 1))
            st = fv.stats()
            res[name] = dict(nseq=nseq, ms_per_call=spread(ms), ms_per_sequence_median=statistics.median(ms) / nseq,
                             top_pass_lockstep_us=spread(step_us), gpu_ms=st["gpu_ms"], step_launches=st["step_launches"],
                             task_steps=st["task_steps"], passes=st["passes"], device_bytes=st["device_bytes"],
                             profiled=profiled(fv, fn))
        # the single decode again under every batch limit (its right-hand generations carry up to that many tasks a launch)
        by_batch = {}
        for mb in (1, 2, 4, 8):
            fv.set_option(decoder.OPT_MAX_BATCH, mb)
            single()
            by_batch[mb] = spread([1e3 * timed(single, args.min_seconds) for _ in range(3)])
            by_batch[mb]["step_launches"] = fv.stats()["step_launches"]
        fv.set_option(decoder.OPT_MAX_BATCH, 8)
        single()
        facts = model_facts(fv, ip[-1])
        facts["set_model_ms"] = set_ms
        step_s = 1e-6 * res["single"]["top_pass_lockstep_us"]["median"]
        floor_s = facts["table_bytes_per_step"] / HBM_BYTES_PER_S + LAUNCH_S
        return dict(K=k, T=T, M=M_SYMBOLS, mean_in_degree=float(ip[-1]) / k, seed=SEED, n_split=N_SPLIT, mode="reference", generator_s=gen_s,
                    dense_table_bytes_fv_set_model_would_need=8 * k * k, model=facts, results=res, single_ms_by_max_batch=by_batch,
                    single_step_us=1e6 * step_s, single_step_streamed_bytes_per_s=facts["table_bytes_per_step"] / step_s,
                    single_step_floor_us=1e6 * floor_s, single_step_fraction_of_floor=floor_s / step_s)
    finally:
        fv.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--large-k", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_model_bench.json"))
    ap.add_argument("--git-head", default="")
    args = ap.parse_args()
    if args.alternations < 5 or args.min_seconds < 0.5:
        print("note: fewer than 5 alternations or less than 0.5 s per timing: not a result to quote", file=sys.stderr)
    out = dict(tool="tools/bench_sparse.py", git_head=git_head(args.git_head), min_seconds=args.min_seconds,
               alternations=args.alternations, hbm_bytes_per_s=HBM_BYTES_PER_S, launch_s=LAUNCH_S)
    out["cfg2"] = part_cfg2(args)
    c = out["cfg2"]
    print(f"cfg2: dense-set sparse walk {c['variants']['dense_set_sparse_q16']['ms_per_decode']['median']:.3f} ms, sparse-set "
          f"{c['variants']['sparse_set_csr']['ms_per_decode']['median']:.3f} ms per decode: x{c['decode_ratio_median']:.3f} "
          f"(streamed bytes x{c['streamed_bytes_ratio']:.3f}, spread {c['run_to_run_range_rel']:.3f})", file=sys.stderr, flush=True)
    if not args.skip_large:
        out["large"] = part_large(args)
        g = out["large"]
        print(f"K={g['K']}: {g['single_step_us']:.1f} us per step, {g['single_step_streamed_bytes_per_s'] / 1e12:.2f} TB/s streamed, "
              f"{g['single_step_fraction_of_floor']:.2f} of the floor; batch of 8: {g['results']['batch8']['ms_per_sequence_median']:.2f} ms per sequence",
              file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
