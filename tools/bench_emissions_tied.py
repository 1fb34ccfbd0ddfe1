#!/usr/bin/env python3
"""bench_emissions_tied.py — what fv_set_emissions costs when the scores arrive as the models that produce them hold
them: 16-bit, and tied (P classes shared by K states through fv_set_emission_map), against today's float32 [T][K] route.

  python tools/bench_emissions_tied.py [--min-seconds 0.5] [--alternations 5] [--skip-large] [--large-k 262144]
                                       [--parent-tree DIR [--parent-head REV]]
                                       [--out profiles/emissions_tied_bench.json] [--git-head REV]

Two shapes, ONE process, one context each: cfg2 (bench.py's model: K = 3965, density 0.112, seed 12; T = 256, P = 512)
and the CSR showcase (K = 262144 (--large-k) with about 32 in-edges per state, data_script.make_model_csr; T = 256,
P = 4096), n_split = 8, FV_MODE_REFERENCE, the library's AUTO kernel.  The class scores are bfloat16 values, so the
three routes stage the same tables: `f32_TK` is the float32 expansion [T][K] (today's route), `bf16_TK` the bfloat16
expansion [T][K], `bf16_TP_map` the bfloat16 block [T][P] through the map.

(a) fv_set_emissions per call, each route from a host pointer and from a device pointer.  First every route is staged
    and decoded once and the decodes are asserted equal (path, score, return code).  Then the routes alternate: each
    timing is a host clock around repeated calls worth at least --min-seconds, --alternations times; per route the
    median and range of ms per call.  (Setting or clearing the map between routes is outside the clock.)
(b) the staging kernels alone through fv_test_stage_emissions_ms (device events around 200 launches back to back, five
    timings each): stage_emissions<TIN, false> over [T][K] and stage_emissions<TIN, true> over [T][P], beside the byte
    floor (bytes read + 12 * T * K) / 8 TB/s + 3 us; bytes read = sizeof(TIN) * T * K, or
    sizeof(TIN) * T * P + 4 * K through the map.
(c) against the parent commit (--parent-tree DIR: a built checkout of it): a child process per tree, alternated three
    times, each timing stage_emissions<float> and <double> through the hook and the cfg2 emission decode
    (decode_full(ob=None), host clock) on that tree's library.  Per figure both trees' medians and ranges, and whether
    the medians differ by no more than the larger run-to-run range of the two.  Without --parent-tree: "not measured".

The JSON goes to --out and to stdout.  There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--probe-tree") + 1]) if "--probe-tree" in sys.argv else ROOT
sys.path.insert(0, TREE)          # (the probe of (c) runs this file on another tree's package)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from flash_viterbi_amd import decoder, hostio  # noqa: E402          (first: bench_emissions puts its own tree in front)
from flash_viterbi_amd.generate_data import data_script  # noqa: E402
from bench_emissions import HBM_BYTES_PER_S, LAUNCH_S, git_head, libm_log, spread, timed  # noqa: E402

K_CFG2, T, M_SYMBOLS, PROB, SEED, N_SPLIT = 3965, 256, 50, 0.112, 12, 8
P_CFG2, P_LARGE = 512, 4096


def bf16_bits(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_to_f32(u):
    return (u.astype(np.uint32) << 16).view(np.float32)


def class_scores(K, P, seed):
    """(map[K], bfloat16 bits [T][P]): finite log scores, every class used"""
    rs = np.random.RandomState(seed)
    pdf = rs.randint(0, P, size=K).astype(np.int32)
    pdf[rs.permutation(K)[:P]] = np.arange(P)
    return pdf, bf16_bits(np.log(rs.uniform(0.05, 1.0, size=(T, P))))


def routes(fv, pdf, U):
    """[(name, prepare, call, input bytes)] and release(); every block is made once, outside every clock"""
    K, P = pdf.size, U.shape[1]
    f32_TK = np.ascontiguousarray(bf16_to_f32(U)[:, pdf])
    bf16_TK = np.ascontiguousarray(U[:, pdf])
    ptrs = [fv.test_device_alloc(a) for a in (f32_TK, bf16_TK, U)]
    no_map, with_map = (lambda: fv.set_emission_map(None)), (lambda: fv.set_emission_map(pdf, P))
    BF = decoder.EMIS_LOG_BF16
    out = [("f32_TK host", no_map, lambda: fv.set_emissions(f32_TK), f32_TK.nbytes),
           ("f32_TK device", no_map, lambda: fv.set_emissions((ptrs[0], np.float32, T, K)), f32_TK.nbytes),
           ("bf16_TK host", no_map, lambda: fv.set_emissions((bf16_TK.ctypes.data, BF, T, K)), bf16_TK.nbytes),
           ("bf16_TK device", no_map, lambda: fv.set_emissions((ptrs[1], BF, T, K)), bf16_TK.nbytes),
           ("bf16_TP_map host", with_map, lambda: fv.set_emissions((U.ctypes.data, BF, T, P)), U.nbytes),
           ("bf16_TP_map device", with_map, lambda: fv.set_emissions((ptrs[2], BF, T, P)), U.nbytes)]

    def release():
        for p in ptrs:
            fv.test_device_free(p)
    return out, release


def kernel_floor(read_bytes, K):
    return 1e6 * ((read_bytes + 12 * T * K) / HBM_BYTES_PER_S + LAUNCH_S)


def stage_kernels(fv, pdf, U, with_f64, reps=200, timings=5):
    """(b): every instantiation through the hook, beside its byte floor"""
    K, P = pdf.size, U.shape[1]
    wide = bf16_to_f32(U)
    forms = {"f32": (wide, np.float32), "f16": (wide.astype(np.float16), np.float16), "bf16": (U, decoder.EMIS_LOG_BF16)}
    if with_f64:
        forms["f64"] = (wide.astype(np.float64), np.float64)
    out = {}
    for tied in (False, True):
        fv.set_emission_map(pdf, P) if tied else fv.set_emission_map(None)
        for tin, (block, dtype) in forms.items():
            block = np.ascontiguousarray(block if tied else block[:, pdf])
            ptr = fv.test_device_alloc(block)
            try:
                us = [1e3 * fv.test_stage_emissions_ms(ptr, dtype, T, block.shape[1], reps) for _ in range(timings)]
            finally:
                fv.test_device_free(ptr)
            read = block.nbytes + (4 * K if tied else 0)
            sp, floor = spread(us), kernel_floor(read, K)
            out[f"stage_emissions<{tin}, {'true' if tied else 'false'}>"] = dict(
                us_per_launch=sp, launches_per_timing=reps, bytes_read=read, bytes_written=12 * T * K, floor_us=floor,
                floor_over_median=floor / sp["median"])
    fv.set_emission_map(None)
    return out


def shape(name, fv, pdf, U, args, with_f64):
    K, P = pdf.size, U.shape[1]
    rt, release = routes(fv, pdf, U)
    try:
        first = None
        for rname, prepare, call, _ in rt:                          # every route decodes the same, exactly
            prepare()
            call()
            path, score, rc = fv.decode_full(None, N_SPLIT, T=T)
            got = (path.tolist(), float(score), rc, fv.stats()["kernel"])
            first = first or got
            assert got == first, f"{name}: the decode after route {rname} differs from the first route's"
        ms = {r[0]: [] for r in rt}
        for _ in range(args.alternations):
            for rname, prepare, call, _ in rt:
                prepare()
                call()
                ms[rname].append(1e3 * timed(call, args.min_seconds))
        staging = {r[0]: dict(ms_per_call=spread(ms[r[0]]), input_bytes=r[3]) for r in rt}
        for rname in ms:
            print(f"{name}: {rname}: {staging[rname]['ms_per_call']['median']:.3f} ms per call", file=sys.stderr, flush=True)
    finally:
        release()
    return dict(K=K, T=T, P=P, table_bytes=12 * T * K, map_bytes=4 * K, decodes_equal=True, decode_kernel=first[3],
                set_emissions=staging, stage_kernels=stage_kernels(fv, pdf, U, with_f64))


def cfg2_model():
    A64, B64, Pi64 = data_script.make_model64(K_CFG2, M_SYMBOLS, SEED, PROB)
    return hostio.quantize_text16(A64), hostio.quantize_text16(B64), hostio.quantize_text16(Pi64)


def probe(args):
    """(c), one tree: the float32 / float64 staging kernels through the hook and the cfg2 emission decode; one JSON line"""
    A, B, Pi = cfg2_model()
    ob = np.asarray(data_script.make_observations(T, M_SYMBOLS, SEED), dtype=np.int32)
    logE = np.ascontiguousarray(libm_log(B)[:, ob].T)
    fv = decoder.FlashViterbi(0)
    out = {}
    try:
        fv.set_model(A, B, Pi)
        for tin, block in (("float", np.ascontiguousarray(logE.astype(np.float32))), ("double", logE)):
            ptr = fv.test_device_alloc(block)
            try:
                out[f"stage_emissions<{tin}> us"] = [1e3 * fv.test_stage_emissions_ms(ptr, block.dtype, T, K_CFG2, 200) for _ in range(5)]
            finally:
                fv.test_device_free(ptr)
        fv.set_emissions(logE)
        run = lambda: fv.decode_full(None, N_SPLIT, T=T)               # noqa: E731
        run()
        out["cfg2 emission decode ms"] = [1e3 * timed(run, args.min_seconds) for _ in range(args.alternations)]
        out["library"] = os.path.relpath(decoder.load_library()._name, TREE)
        out["path_crc"] = int(np.bitwise_xor.reduce(run()[0] * np.arange(1, T + 1, dtype=np.int32)))
    finally:
        fv.close()
    print("PROBE " + json.dumps(out))


def against_parent(args, rounds=3):
    if not args.parent_tree:
        return dict(status="not measured", reason="no --parent-tree")
    got = {"parent": {}, "this": {}}
    for _ in range(rounds):
        for who, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--probe-tree", tree, "--min-seconds", str(args.min_seconds),
                                  "--alternations", str(args.alternations)], capture_output=True, text=True, timeout=600, cwd=tree)
            if res.returncode != 0:
                raise RuntimeError(f"the probe of {tree} ended with {res.returncode}:\n{res.stderr[-1500:]}")
            line = next(ln for ln in res.stdout.splitlines() if ln.startswith("PROBE "))
            for k, v in json.loads(line[6:]).items():
                got[who].setdefault(k, []).extend(v if isinstance(v, list) else [v])
    assert not any(lib.startswith("..") for who in got for lib in got[who]["library"]), "a probe loaded a library outside its tree"
    assert set(got["parent"]["path_crc"]) == set(got["this"]["path_crc"]) and len(set(got["this"]["path_crc"])) == 1, "the trees decode differently"
    figures = {}
    for k in got["this"]:
        if k in ("path_crc", "library"):
            continue
        a, b = spread(got["parent"][k]), spread(got["this"][k])
        rng = max(a["range_rel"], b["range_rel"])
        diff = abs(b["median"] - a["median"]) / a["median"]
        figures[k] = dict(parent=a, this=b, this_over_parent_median=b["median"] / a["median"], larger_run_to_run_range_rel=rng,
                          medians_differ_rel=diff, within_range=diff <= rng)
        print(f"(c) {k}: parent {a['median']:.4f}, this {b['median']:.4f} (range {rng:.4f})", file=sys.stderr, flush=True)
    return dict(status="measured", parent_head=args.parent_head or "not given", rounds=rounds, paths_equal=True, figures=figures)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--large-k", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emissions_tied_bench.json"))
    ap.add_argument("--git-head", default="")
    ap.add_argument("--parent-tree", default="", metavar="DIR", help="a built checkout of the parent commit, for (c)")
    ap.add_argument("--parent-head", default="", metavar="REV")
    ap.add_argument("--probe-tree", default="", metavar="DIR", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.probe_tree:
        probe(args)
        return
    if args.alternations < 5 or args.min_seconds < 0.5:
        print("note: fewer than 5 alternations or less than 0.5 s per timing: not a result to quote", file=sys.stderr)
    out = dict(tool="tools/bench_emissions_tied.py", git_head=git_head(args.git_head), min_seconds=args.min_seconds,
               alternations=args.alternations, hbm_bytes_per_s=HBM_BYTES_PER_S, launch_s=LAUNCH_S, n_split=N_SPLIT, mode="reference")
    A, B, Pi = cfg2_model()
    fv = decoder.FlashViterbi(0)
    try:
        fv.set_model(A, B, Pi)
        out["cfg2"] = shape("cfg2", fv, *class_scores(K_CFG2, P_CFG2, SEED), args, with_f64=True)
    finally:
        fv.close()
    if args.skip_large:
        out["csr_showcase"] = dict(status="not measured", reason="--skip-large")
    else:
        ip, ix, dt, B, Pi = data_script.make_model_csr(args.large_k, M_SYMBOLS, SEED, 32)
        fv = decoder.FlashViterbi(0)
        try:
            fv.set_model_sparse(ip, ix, dt, B, Pi)
            out["csr_showcase"] = shape("csr_showcase", fv, *class_scores(args.large_k, P_LARGE, SEED + 1), args, with_f64=False)
            out["csr_showcase"]["in_edges_per_state"] = float(ix.size) / args.large_k
        finally:
            fv.close()
    out["against_parent"] = against_parent(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
