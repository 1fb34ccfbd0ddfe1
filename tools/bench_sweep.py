"""The packed kernel's block-minimum sweep and code-free single-task form, measured against a built checkout of the parent:
    python tools/bench_sweep.py --parent-tree DIR [--out profiles/sweep_tree_ab.json] [--rounds 5]

`python bench.py`, `--workload cfg3` and `--workload cfg4` from the parent tree and from this one, alternated `rounds` times in
one visit: ms_per_step, forward_pass_ms and roofline.launch_us of each run; beside them one process per tree and round that
decodes cfg2 and cfg3 and reads the right-hand part (gpu_ms - top_pass_ms) and the three refine counters; the --dump-outputs
files of the two trees compared.  Bar (the project's usual one):
  cfg2, cfg3  the branch's maximum ms_per_step below the parent's minimum; outputs identical; refine_near / refine_rescan /
              refine_saturated equal (the parent is the reference);
  cfg4        FLASH-BS, untouched: the branch's median inside the parent's min-max range.
Every child process runs under a time limit and the script stops at the first one that fails."""
import argparse, json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    rh, top = [], []
    for _ in range(W["steps"]):
        fv.decode_full(ob, bench.N_SPLIT); st = fv.stats()
        rh.append(st["gpu_ms"] - st["top_pass_ms"]); top.append(st["top_pass_ms"])
    out[w] = {"right_ms": float(np.median(rh)), "top_pass_ms": float(np.median(top)),
              "counters": [int(st["refine_near"]), int(st["refine_rescan"]), int(st["refine_saturated"])]}
fv.close()
print(json.dumps(out))
'''
DENSE, ALL = ("cfg2", "cfg3"), ("cfg2", "cfg3", "cfg4")


def child(cmd, cwd, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"FAILED ({p.returncode}) in {cwd}: {' '.join(cmd)}\n{p.stderr[-1500:]}")
    return p.stdout.strip().splitlines()[-1]


def alternate(parent_tree, rounds):
    trees = {"parent": os.path.abspath(parent_tree), "branch": ROOT}
    keys = ("ms_per_step", "forward_pass_ms", "launch_us", "right_ms", "top_pass_ms")
    runs = {w: {t: {k: [] for k in keys} for t in trees} for w in ALL}
    counters = {w: {t: None for t in trees} for w in DENSE}
    with tempfile.TemporaryDirectory() as tmp:
        for it in range(rounds):
            for t, d in trees.items():
                for w in ALL:
                    line = json.loads(child([sys.executable, "bench.py", "--workload", w, "--dump-outputs", os.path.join(tmp, t + w)], d, 240))
                    runs[w][t]["ms_per_step"].append(line["ms_per_step"])
                    runs[w][t]["forward_pass_ms"].append(line.get("forward_pass_ms"))
                    runs[w][t]["launch_us"].append(line.get("roofline", {}).get("launch_us"))
                r = json.loads(child([sys.executable, "-c", RIGHT_MS], d, 240))
                for w in DENSE:
                    runs[w][t]["right_ms"].append(r[w]["right_ms"]); runs[w][t]["top_pass_ms"].append(r[w]["top_pass_ms"])
                    counters[w][t] = r[w]["counters"]
                print(it, t, {w: runs[w][t]["ms_per_step"][-1] for w in ALL}, r, flush=True)
        out = {}
        for w in ALL:
            p, b = runs[w]["parent"]["ms_per_step"], runs[w]["branch"]["ms_per_step"]
            same = all(np.array_equal(np.load(os.path.join(tmp, "parent" + w, n + ".npy")), np.load(os.path.join(tmp, "branch" + w, n + ".npy")))
                       for n in ("path", "score", "rc"))
            med = {t: {k: statistics.median(v) for k, v in runs[w][t].items() if v and v[0] is not None} for t in trees}
            out[w] = {"command": "python bench.py" + ("" if w == "cfg2" else " --workload " + w), "parent": runs[w]["parent"], "branch": runs[w]["branch"],
                      "parent_min": min(p), "parent_max": max(p), "parent_median": statistics.median(p),
                      "branch_min": min(b), "branch_max": max(b), "branch_median": statistics.median(b),
                      "ratio_of_medians": statistics.median(b) / statistics.median(p), "medians": med, "dump_outputs_identical": bool(same)}
            if w in DENSE:
                out[w]["refine_near_rescan_saturated"] = counters[w]
                out[w]["counters_equal"] = counters[w]["parent"] == counters[w]["branch"]
                out[w]["branch_max_below_parent_min"] = max(b) < min(p)
                out[w]["gain_over_parent_spread"] = (statistics.median(p) - statistics.median(b)) / max(max(p) - min(p), 1e-12)
                out[w]["pass"] = bool(max(b) < min(p) and same and out[w]["counters_equal"])
            else:
                out[w]["branch_median_inside_parent_range"] = min(p) <= statistics.median(b) <= max(p)
                out[w]["pass"] = bool(out[w]["branch_median_inside_parent_range"] and same)
    return out


def git_head(d):
    p = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=d, capture_output=True, text=True)
    return p.stdout.strip() or "unknown"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_tree_ab.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--head", default=None, help="this tree's commit, where it is a copy without .git")
    ap.add_argument("--parent-head", default=None, help="the parent's commit, where the parent tree is an export without .git")
    a = ap.parse_args()
    doc = {"what": "block-minimum sweep + code-free single-task form of trellis_step_u16: tools/bench_sweep.py",
           "head": a.head or git_head(ROOT), "parent_head": a.parent_head or git_head(a.parent_tree), "rounds": a.rounds,
           "workloads": alternate(a.parent_tree, a.rounds)}
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({w: {k: v for k, v in d.items() if not isinstance(v, (list, dict))} for w, d in doc["workloads"].items()}, indent=1))
