"""FV_OPT_FLAT_GENERATIONS measured: python tools/bench_flat.py [--parent-tree DIR] [--out profiles/flat_generations_ab.json]

  (a) auto threshold on K: K = 512, 1024, 2048 and the bench model (K = 3965) at T = 256, n_split = 8, the option at 0 and 2
      alternated five times in one process: host wall ms per decode, median gpu_ms - top_pass_ms, step launches, misses;
  (b) auto bound on T: the bench model at T = 512, 1024, 2048, the same alternation three times;
  (c) with --parent-tree (a built checkout of the parent commit): `python bench.py` and `python bench.py --workload cfg3`
      from the parent tree and from this one, alternated five times, ms_per_step of each run; beside it a run of the same
      two workloads that reads gpu_ms - top_pass_ms and the misses over the timed steps; the --dump-outputs files of the
      two trees compared.  Pass: cfg2 — the branch's maximum below the parent's minimum; cfg3 — the branch's median not
      above the parent's maximum.
Every child process runs under a time limit and the script stops at the first one that fails."""
import argparse, json, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

RIGHT_MS = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
import numpy as np, bench
from flash_viterbi_amd import decoder
out, fv = {}, None
for w in ("cfg2", "cfg3"):
    W = bench.WORKLOADS[w]
    ob = np.asarray(bench.data_script.make_observations(W["T"], bench.M_SYMBOLS, bench.SEED), dtype=np.int32)
    if fv is None:
        _, model, _ = bench.build_workload(W)
        fv = decoder.FlashViterbi(0); fv.set_model(*model); fv.set_option(decoder.OPT_KERNEL, bench.DENSE_KERNEL)
    for _ in range(W["warmup"]): fv.decode_full(ob, bench.N_SPLIT)
    rh, missed, flat = [], 0, 0
    for _ in range(W["steps"]):
        fv.decode_full(ob, bench.N_SPLIT); st = fv.stats()
        rh.append(st["gpu_ms"] - st["top_pass_ms"]); missed += st.get("flat_missed", 0); flat += st.get("flat_passes", 0)
    out[w] = {"right_ms_median": float(np.median(rh)), "missed_over_timed_steps": missed, "flat_passes_over_timed_steps": flat}
fv.close()
print(json.dumps(out))
'''


def measure(fv, ob, n, flat, reps):
    from flash_viterbi_amd import decoder
    fv.set_option(decoder.OPT_FLAT_GENERATIONS, flat)
    for _ in range(3): fv.decode_full(ob, n)
    rh = []; t0 = time.perf_counter()
    for _ in range(reps):
        fv.decode_full(ob, n); s = fv.stats(); rh.append(s["gpu_ms"] - s["top_pass_ms"])
    return dict(flat=flat, wall_ms=(time.perf_counter() - t0) / reps * 1e3, right_ms=float(np.median(rh)), launches=s["step_launches"],
                flat_passes=s["flat_passes"], missed=s["flat_missed"])


def in_process():
    import modelgen
    from flash_viterbi_amd import decoder
    by_k, by_t = {}, []
    for K in (512, 1024, 2048, 3965):
        A, B, Pi, ob = modelgen.model32(dict(kind="data_script", K=K, M=50, T=2048 if K == 3965 else 256, prob=0.112, seed=12))
        fv = decoder.FlashViterbi(0); fv.set_model(A, B, Pi); fv.set_option(decoder.OPT_KERNEL, decoder.KERNEL_U16_REFINE)
        by_k[f"K{K}"] = [measure(fv, ob[:256], 8, f, 40) for f in (0, 2) * 5]
        print(K, json.dumps(by_k[f"K{K}"]), flush=True)
        if K == 3965:
            for T in (512, 1024, 2048):
                by_t += [dict(T=T, **measure(fv, ob[:T], 8, f, 12)) for f in (0, 2) * 3]
            print(json.dumps(by_t), flush=True)
        fv.close()
    return by_k, by_t


def child(cmd, cwd, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"FAILED ({p.returncode}) in {cwd}: {' '.join(cmd)}\n{p.stderr[-1500:]}")
    return p.stdout.strip().splitlines()[-1]


def alternate(parent_tree):
    trees = {"parent": os.path.abspath(parent_tree), "branch": ROOT}
    runs = {w: {t: [] for t in trees} for w in ("cfg2", "cfg3")}
    right = {w: {t: [] for t in trees} for w in ("cfg2", "cfg3")}
    missed = {"cfg2": 0, "cfg3": 0}
    with tempfile.TemporaryDirectory() as tmp:
        for it in range(5):
            for t, d in trees.items():
                for w in runs:
                    line = json.loads(child([sys.executable, "bench.py", "--workload", w, "--dump-outputs", os.path.join(tmp, t + w)], d, 240))
                    runs[w][t].append(line["ms_per_step"])
                r = json.loads(child([sys.executable, "-c", RIGHT_MS], d, 240))
                for w in runs:
                    right[w][t].append(r[w]["right_ms_median"])
                    missed[w] += r[w]["missed_over_timed_steps"] if t == "branch" else 0
                print(it, t, {w: runs[w][t][-1] for w in runs}, r, flush=True)
        out = {}
        for w in runs:
            p, b = runs[w]["parent"], runs[w]["branch"]
            same = all(np.array_equal(np.load(os.path.join(tmp, "parent" + w, n + ".npy")), np.load(os.path.join(tmp, "branch" + w, n + ".npy")))
                       for n in ("path", "score", "rc"))
            out[w] = {"command": "python bench.py" + ("" if w == "cfg2" else " --workload cfg3"), "metric": "ms_per_step", "parent": p, "branch": b,
                      "parent_min": min(p), "parent_max": max(p), "parent_median": statistics.median(p),
                      "branch_min": min(b), "branch_max": max(b), "branch_median": statistics.median(b),
                      "branch_max_below_parent_min": max(b) < min(p), "branch_median_not_above_parent_max": statistics.median(b) <= max(p),
                      "ratio_of_medians": statistics.median(b) / statistics.median(p), "right_hand_ms": right[w],
                      "flat_missed_over_timed_steps": missed[w], "dump_outputs_identical": bool(same)}
    return out


def git_head(d):
    p = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=d, capture_output=True, text=True)
    return p.stdout.strip() or "unknown"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_generations_ab.json"))
    a = ap.parse_args()
    by_k, by_t = in_process()
    doc = {"what": "FV_OPT_FLAT_GENERATIONS: tools/bench_flat.py", "head": git_head(ROOT), "auto_threshold_K": by_k, "auto_bound_T": by_t}
    if a.parent_tree:
        doc["workloads"] = alternate(a.parent_tree)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({w: {k: v for k, v in d.items() if not isinstance(v, (list, dict))} for w, d in doc.get("workloads", {}).items()}, indent=1))
