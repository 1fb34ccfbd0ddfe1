#!/usr/bin/env python3
"""bench_stream_lag.py — fv_set_max_lag, the lag-bounded online decode, beside the unbounded stream on the same box
(DESIGN.md 5.6c).  One process; the variants of a workload are alternated, at least --min-seconds each, --alternations
times; medians and ranges.

  python tools/bench_stream_lag.py [--min-seconds 0.5] [--alternations 5] [--skip-large] [--large-k 262144] [--large-t 512]
                                   [--parent-root DIR] [--out profiles/stream_lag_bench.json] [--git-head REV]
  python tools/bench_stream_lag.py --unbounded-child DIR      # the unbounded figures of the built checkout DIR, as JSON, nothing else

Workloads: cfg3 (bench.py's model, K = 3965, set dense under the default kernel, T = 4096), a CSR-set model of K =
--large-k with about 32 in-edges per state (T = --large-t), and `rotor`, a permutation model of K = 3965 (T = 4096) whose
survivor paths never merge: without a bound nothing commits before the close.  Per workload, in pushes of 64:
  single        one stream at (max_lag, check_every) = (0, 16), (64, 16), (16, 16): wall time per consumed time — open,
                pushes and close included — forced commits, pruned states, the largest pending count after a push, the
                arg rows allocated and their bytes;
  set_of_8      the same for eight slots pushed together (the sequence rolled per slot): wall time per time index, in which
                all eight slots advance; the counts are slot 0's.
--parent-root: a built checkout of the parent commit (its flash_viterbi_amd package with libflashvit.so is enough).  The
unbounded stream and set (K = 3965, T = 4096, pushes of 16 and 64) are then timed in child processes that import the
parent's package and this tree's alternately; the medians must lie within each other's run-to-run range, else the
unbounded path has been touched.

The JSON goes to --out and to stdout.  There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--unbounded-child" in sys.argv[1:-1]:      # a child: the package of the checkout it is given, imported before anything else
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--unbounded-child") + 1]))
    import flash_viterbi_amd  # noqa: E402,F401
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_sparse import K, M_SYMBOLS, PROB, SEED, git_head, spread, timed  # noqa: E402

GRID = ((0, 16), (64, 16), (16, 16))
SLOTS = 8


def load():
    """the package (a child: the one imported at the top)"""
    from flash_viterbi_amd import decoder, hostio
    from flash_viterbi_amd.generate_data import data_script
    return decoder, hostio, data_script


def dense_context(mods):
    decoder, hostio, data_script = mods
    A64, B64, Pi64 = data_script.make_model64(K, M_SYMBOLS, SEED, PROB)
    fv = decoder.FlashViterbi(0)
    fv.set_model(hostio.quantize_text16(A64), hostio.quantize_text16(B64), hostio.quantize_text16(Pi64))
    return fv


def rotor_context(mods):
    """state s moves to s + 1 with probability 1: K chains that never meet"""
    decoder = mods[0]
    rs = np.random.RandomState(SEED)
    A = np.zeros((K, K), dtype=np.float32)
    A[np.arange(K), (np.arange(K) + 1) % K] = 1
    B = rs.uniform(0.05, 1.0, (K, M_SYMBOLS)).astype(np.float32)
    B /= B.sum(axis=1, keepdims=True)
    fv = decoder.FlashViterbi(0)
    fv.set_model(A, B, np.full(K, 1.0 / K, dtype=np.float32))
    return fv


def stream_once(fv, ob, push, check_every):
    fv.stream_open(0, check_every)
    worst = 0
    for pos in range(0, ob.size, push):
        fv.stream_push(ob=ob[pos:pos + push])
        worst = max(worst, fv.stream_pending())
    _, score, rc = fv.stream_close()
    return worst, rc


def set_once(fv, obs, push, check_every):
    fv.streams_open(len(obs), 0, check_every)
    ids, worst = list(range(len(obs))), 0
    for pos in range(0, obs[0].size, push):
        fv.streams_push(ids, obs=[o[pos:pos + push] for o in obs])
        worst = max(worst, max(fv.streams_pending(s) for s in ids))
    rcs = [fv.streams_close(s)[2] for s in ids]
    fv.streams_end()
    return worst, min(rcs)


def measure(fv, ob, args, push=64):
    """single stream and set of SLOTS at every (max_lag, check_every) of GRID, alternated"""
    T = ob.size
    obs = [np.ascontiguousarray(np.roll(ob, 37 * s)) for s in range(SLOTS)]
    variants, facts = {}, {}
    for L, C in GRID:
        variants[("single", L, C)] = lambda C=C: stream_once(fv, ob, push, C)
        variants[("set_of_8", L, C)] = lambda C=C: set_once(fv, obs, push, C)
    for key, fn in variants.items():                             # warm, and what the run counts
        fv.set_max_lag(key[1])
        worst, rc = fn()
        # (the stream just closed; slot 0 of the set just ended)
        st, lag = (fv.stream_stats(), fv.lag_stats()) if key[0] == "single" else (None, fv.lag_stats(0))
        facts[key] = dict(max_lag=key[1], check_every=key[2], rc=rc, largest_pending=worst, forced_commits=lag["forced_commits"],
                          pruned_states=lag["pruned_states"], first_forced_time=lag["first_forced_time"])
        if st:
            facts[key].update(checks=st["checks"], commits=st["commits"], arg_rows_capacity=st["arg_rows_capacity"],
                              regrows=st["regrows"], kernel=st["kernel"])
        else:
            ss = fv.streams_stats()
            facts[key].update(check_launches=ss["check_launches"], check_slots=ss["check_slots"], kernel=ss["kernel"])
    wall = {key: [] for key in variants}
    for _ in range(args.alternations):
        for key, fn in variants.items():
            fv.set_max_lag(key[1])
            wall[key].append(1e6 * timed(fn, args.min_seconds) / T)
    fv.set_max_lag(0)
    out = dict(T=T, push=push)
    for group in ("single", "set_of_8"):
        out[group] = {}
        base = spread(wall[(group, 0, 16)])["median"]
        for key in variants:
            if key[0] == group:
                w = spread(wall[key])
                out[group][f"L{key[1]}_C{key[2]}"] = dict(wall_us_per_time=w, ratio_to_unbounded=w["median"] / base, **facts[key])
    return out


def unbounded_child():
    """the unbounded stream and set at K = 3965, T = 4096 on the imported package: wall us per time index, pushes of 16 and 64"""
    mods = load()
    fv = dense_context(mods)
    try:
        ob = np.asarray(mods[2].make_observations(4096, M_SYMBOLS, SEED), dtype=np.int32)
        obs = [np.ascontiguousarray(np.roll(ob, 37 * s)) for s in range(SLOTS)]
        out = {}
        for push in (16, 64):
            for name, fn in (("single", lambda: stream_once(fv, ob, push, 0)), ("set_of_8", lambda: set_once(fv, obs, push, 0))):
                fn()
                out[f"{name}_push_{push}"] = 1e6 * timed(fn, 0.5) / ob.size
        print(json.dumps(out))
    finally:
        fv.close()


def against_parent(parent_root, alternations):
    runs = {"parent": [], "this": []}
    for _ in range(alternations):
        for who, root in (("parent", parent_root), ("this", ROOT)):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--unbounded-child", root], capture_output=True,
                                 text=True, timeout=600)
            if res.returncode != 0:
                return dict(status="not measured", reason=f"child on {who}: exit {res.returncode}", stderr=res.stderr[-600:])
            runs[who].append(json.loads(res.stdout.strip().splitlines()[-1]))
    out = dict(status="measured", workload="K = 3965 dense, T = 4096, max_lag = 0, default check interval", alternations=alternations)
    for key in runs["this"][0]:
        p, t = spread([r[key] for r in runs["parent"]]), spread([r[key] for r in runs["this"]])
        out[key] = dict(parent_us_per_time=p, this_us_per_time=t, ratio=t["median"] / p["median"],
                        within_run_to_run_range=bool(t["min"] <= p["max"] and p["min"] <= t["max"]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--large-k", type=int, default=262144)
    ap.add_argument("--large-t", type=int, default=512)
    ap.add_argument("--parent-root", default="", metavar="DIR")
    ap.add_argument("--unbounded-child", default="", metavar="DIR")
    ap.add_argument("--only-parent", action="store_true", help="only the comparison with --parent-root, merged into the record at --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_lag_bench.json"))
    ap.add_argument("--git-head", default="")
    args = ap.parse_args()
    if args.unbounded_child:
        unbounded_child()
        return
    if args.only_parent:
        with open(args.out) as fh:
            out = json.load(fh)
        out["unbounded_against_parent"] = against_parent(args.parent_root, args.alternations)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out["unbounded_against_parent"]))
        return
    if args.alternations < 5 or args.min_seconds < 0.5:
        print("note: fewer than 5 alternations or less than 0.5 s per timing: not a result to quote", file=sys.stderr)
    mods = load()
    decoder, _, data_script = mods
    out = dict(tool="tools/bench_stream_lag.py", git_head=git_head(args.git_head), min_seconds=args.min_seconds,
               alternations=args.alternations, slots=SLOTS)
    ob = np.asarray(data_script.make_observations(4096, M_SYMBOLS, SEED), dtype=np.int32)
    for name, make, what in (("cfg3", dense_context, "dense-set, FV_KERNEL_AUTO"),
                             ("rotor", rotor_context, "dense-set permutation model (nothing ever merges), FV_KERNEL_AUTO")):
        fv = make(mods)
        try:
            out[name] = dict(K=K, M=M_SYMBOLS, model=what, arg_row_bytes=4 * K, **measure(fv, ob, args))
        finally:
            fv.close()
        print(f"{name}: done", file=sys.stderr, flush=True)
    if not args.skip_large:
        ip, ix, dt, B, Pi = data_script.make_model_csr(args.large_k, M_SYMBOLS, SEED, 32)
        obl = np.random.RandomState(SEED).randint(0, M_SYMBOLS, args.large_t).astype(np.int32)
        fv = decoder.FlashViterbi(0)
        try:
            fv.set_model_sparse(ip, ix, dt, B, Pi)
            out["large"] = dict(K=args.large_k, M=M_SYMBOLS, mean_in_degree=float(ip[-1]) / args.large_k, model="CSR-set, FV_KERNEL_AUTO",
                                arg_row_bytes=4 * args.large_k, **measure(fv, obl, args))
        finally:
            fv.close()
        print("large: done", file=sys.stderr, flush=True)
    if args.parent_root:
        out["unbounded_against_parent"] = against_parent(args.parent_root, args.alternations)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
