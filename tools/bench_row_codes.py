"""FV_OPT_ROW_CODES measured: python tools/bench_row_codes.py [--parent-tree DIR] [--out profiles/row_codes_ab.json]

  (a) launch families: the bench model (K = 3965, T = 256, n_split = 8) with the option at 0, 3 (single-task launches only: the
      whole-sequence pass), 4 (batched launches only: the right-hand passes) and 2 (both), alternated five times in one
      process: host wall ms per decode, median top_pass_ms and gpu_ms - top_pass_ms, refine candidates (counters[0]) and
      lane rescans per decode.  Auto takes a family if its own setting beats 0 in the part of the decode it changes;
  (b) auto threshold on K: K = 512, 1024, 2048 at T = 256, the option at 0, 4 and 2, the same alternation;
  (c) with --parent-tree (a built checkout of the parent commit): `python bench.py` and `python bench.py --workload cfg3`
      from the parent tree and from this one, alternated five times: ms_per_step, forward_pass_ms and roofline.launch_us of
      each run, beside it a run of the same two workloads that reads gpu_ms - top_pass_ms; the --dump-outputs files of the two
      trees compared.  Pass: cfg2 — the branch's maximum ms_per_step below the parent's minimum; cfg3 — the branch's median
      within the parent's own range or below it.
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
    rh, near = [], []
    for _ in range(W["steps"]):
        fv.decode_full(ob, bench.N_SPLIT); st = fv.stats()
        rh.append(st["gpu_ms"] - st["top_pass_ms"]); near.append(st["refine_near"])
    out[w] = {"right_ms_median": float(np.median(rh)), "refine_candidates_per_decode": float(np.median(near))}
fv.close()
print(json.dumps(out))
'''


def measure(fv, ob, n, opt, reps):
    from flash_viterbi_amd import decoder
    fv.set_option(decoder.OPT_ROW_CODES, opt)
    for _ in range(3): fv.decode_full(ob, n)
    top, rh = [], []; t0 = time.perf_counter()
    for _ in range(reps):
        fv.decode_full(ob, n); s = fv.stats(); top.append(s["top_pass_ms"]); rh.append(s["gpu_ms"] - s["top_pass_ms"])
    return dict(option=opt, wall_ms=(time.perf_counter() - t0) / reps * 1e3, top_pass_ms=float(np.median(top)), right_ms=float(np.median(rh)),
                refine_candidates=s["refine_near"], lane_rescans=s["refine_rescan"], launches=s["step_launches"])


def in_process():
    import modelgen
    from flash_viterbi_amd import decoder
    families, by_k = [], {}
    for K in (3965, 512, 1024, 2048):
        A, B, Pi, ob = modelgen.model32(dict(kind="data_script", K=K, M=50, T=256, prob=0.112, seed=12))
        fv = decoder.FlashViterbi(0); fv.set_model(A, B, Pi); fv.set_option(decoder.OPT_KERNEL, decoder.KERNEL_U16_REFINE)
        if K == 3965:
            families = [measure(fv, ob, 8, o, 40) for o in (0, 3, 4, 2) * 5]
            print(K, json.dumps(families), flush=True)
        else:
            by_k[f"K{K}"] = [measure(fv, ob, 8, o, 40) for o in (0, 4, 2) * 5]
            print(K, json.dumps(by_k[f"K{K}"]), flush=True)
        fv.close()
    med = lambda o, key: statistics.median(r[key] for r in families if r["option"] == o)
    verdict = {"single_task_launches": {"top_pass_ms_off": med(0, "top_pass_ms"), "top_pass_ms_on": med(3, "top_pass_ms"), "wins": med(3, "top_pass_ms") < med(0, "top_pass_ms")},
               "batched_launches": {"right_ms_off": med(0, "right_ms"), "right_ms_on": med(4, "right_ms"), "wins": med(4, "right_ms") < med(0, "right_ms")},
               "both": {"wall_ms_off": med(0, "wall_ms"), "wall_ms_on": med(2, "wall_ms")},
               "refine_candidates_per_decode": {"off": med(0, "refine_candidates"), "on": med(2, "refine_candidates")},
               "lane_rescans_per_decode": {"off": med(0, "lane_rescans"), "on": med(2, "lane_rescans")}}
    return families, verdict, by_k


def child(cmd, cwd, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"FAILED ({p.returncode}) in {cwd}: {' '.join(cmd)}\n{p.stderr[-1500:]}")
    return p.stdout.strip().splitlines()[-1]


def alternate(parent_tree):
    trees = {"parent": os.path.abspath(parent_tree), "branch": ROOT}
    keys = ("ms_per_step", "forward_pass_ms", "launch_us", "right_ms")
    runs = {w: {t: {k: [] for k in keys} for t in trees} for w in ("cfg2", "cfg3")}
    cand = {w: {t: None for t in trees} for w in runs}
    with tempfile.TemporaryDirectory() as tmp:
        for it in range(5):
            for t, d in trees.items():
                for w in runs:
                    line = json.loads(child([sys.executable, "bench.py", "--workload", w, "--dump-outputs", os.path.join(tmp, t + w)], d, 240))
                    runs[w][t]["ms_per_step"].append(line["ms_per_step"]); runs[w][t]["forward_pass_ms"].append(line["forward_pass_ms"])
                    runs[w][t]["launch_us"].append(line["roofline"]["launch_us"])
                r = json.loads(child([sys.executable, "-c", RIGHT_MS], d, 240))
                for w in runs:
                    runs[w][t]["right_ms"].append(r[w]["right_ms_median"]); cand[w][t] = r[w]["refine_candidates_per_decode"]
                print(it, t, {w: runs[w][t]["ms_per_step"][-1] for w in runs}, r, flush=True)
        out = {}
        for w in runs:
            p, b = runs[w]["parent"]["ms_per_step"], runs[w]["branch"]["ms_per_step"]
            same = all(np.array_equal(np.load(os.path.join(tmp, "parent" + w, n + ".npy")), np.load(os.path.join(tmp, "branch" + w, n + ".npy")))
                       for n in ("path", "score", "rc"))
            out[w] = {"command": "python bench.py" + ("" if w == "cfg2" else " --workload cfg3"), "parent": runs[w]["parent"], "branch": runs[w]["branch"],
                      "parent_min": min(p), "parent_max": max(p), "parent_median": statistics.median(p),
                      "branch_min": min(b), "branch_max": max(b), "branch_median": statistics.median(b),
                      "branch_max_below_parent_min": max(b) < min(p), "branch_median_not_above_parent_max": statistics.median(b) <= max(p),
                      "ratio_of_medians": statistics.median(b) / statistics.median(p),
                      "medians": {t: {k: statistics.median(runs[w][t][k]) for k in keys} for t in trees},
                      "refine_candidates_per_decode": cand[w], "dump_outputs_identical": bool(same)}
    return out


def git_head(d):
    p = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=d, capture_output=True, text=True)
    return p.stdout.strip() or "unknown"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_codes_ab.json"))
    a = ap.parse_args()
    families, verdict, by_k = in_process()
    doc = {"what": "FV_OPT_ROW_CODES: tools/bench_row_codes.py", "head": git_head(ROOT),
           "auto_takes": "batched launches of the packed kernel only (the single-task launches of the whole-sequence pass lose), fv_decode_full of one sequence, K >= 2048 (fv_full.hip: ROW_CODES_AUTO_FAMILIES, ROW_CODES_AUTO_MIN_K)",
           "launch_families_K3965": verdict, "launch_families_runs": families, "auto_threshold_K": by_k}
    if a.parent_tree:
        doc["workloads"] = alternate(a.parent_tree)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(verdict, indent=1))
    print(json.dumps({w: {k: v for k, v in d.items() if not isinstance(v, (list, dict))} for w, d in doc.get("workloads", {}).items()}, indent=1))
