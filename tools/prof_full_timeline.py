"""Timeline of one full-state decode out of a rocprofv3 kernel trace of tools/time_kernels.py: per generation, per lock-step
wall time, busy time and launches, and the right-hand part (everything after the whole-sequence pass's back-track) as a
whole: span, step launches, how many of them run at once, idle time.
   python tools/prof_full_timeline.py results.db [decode index from the end] [--json out.json --label NAME]
--json adds the right-hand figures of the decode to out.json under NAME (the file is created or extended)."""
import collections, json, os, sqlite3, sys
import numpy as np
args = [a for a in sys.argv[1:]]
out_json = label = None
if "--json" in args:
    i = args.index("--json"); out_json = args[i + 1]; del args[i:i + 2]
if "--label" in args:
    i = args.index("--label"); label = args[i + 1]; del args[i:i + 2]
db = sqlite3.connect(args[0])
rows = list(db.cursor().execute("select name, start, end from kernels order by start"))
names = [r[0] for r in rows]; st = np.array([r[1] for r in rows], dtype=np.int64); en = np.array([r[2] for r in rows], dtype=np.int64)
short = lambda n: n.split("(")[0].replace("void ", "")[:44]
# a decode = from a clear_outputs (the decode prologue) up to the next one; its generation 0 ends with the back-track
# that follows final_argmax
starts = [i for i, n in enumerate(names) if "clear_outputs" in n]
which = int(args[1]) if len(args) > 1 else -2
i0 = starts[which]; i_end = starts[which + 1] if which + 1 < len(starts) and which != -1 else len(names)
inits = [i for i in range(i0, i_end) if "init_rows" in names[i]]
print(f"decode: kernels {i0}..{i_end}, wall {(en[i0:i_end].max() - st[i0]) / 1e6:.3f} ms, {len(inits)} init_rows launches")
for g, a in enumerate(inits):
    b = inits[g + 1] if g + 1 < len(inits) else i_end
    wall = (en[a:b].max() - st[a]) / 1e3
    busy = (en[a:b] - st[a:b]).sum() / 1e3
    cnt = collections.Counter(short(n) for n in names[a:b])
    tot = collections.defaultdict(float)
    for i in range(a, b): tot[short(names[i])] += (en[i] - st[i]) / 1e3
    print(f" init_rows {g}: {b - a:4d} kernels wall {wall:8.1f} us, summed kernel time {busy:8.1f} us")
    for k, v in sorted(tot.items(), key=lambda x: -x[1])[:5]: print(f"      {k:44s} {cnt[k]:4d} x {v / cnt[k]:6.1f} us")


def union_us(idx):
    """time covered by at least one of the kernels idx (us)"""
    cover, hi = 0, None
    for i in sorted(idx, key=lambda j: st[j]):
        if hi is None or st[i] > hi: cover += en[i] - st[i]; hi = en[i]
        elif en[i] > hi: cover += en[i] - hi; hi = en[i]
    return cover / 1e3


# the right-hand part: after generation 0's back-track, up to the result block
argmax = next(i for i in range(i0, i_end) if "final_argmax" in names[i])
r0 = next(i for i in range(argmax, i_end) if "backtrack" in names[i]) + 1
r1 = next((i for i in range(r0, i_end) if "pack_result" in names[i]), i_end)
idx = list(range(r0, r1))
steps = [i for i in idx if "trellis_step" in names[i]]
span = (en[idx].max() - en[r0 - 1]) / 1e3
step_sum = float((en[steps] - st[steps]).sum() / 1e3)
right = {
    "span_us": float(span), "kernels": len(idx), "step_launches": len(steps),
    "step_mean_us": step_sum / max(len(steps), 1),
    "steps_running_at_once_mean": step_sum / max(union_us(steps), 1e-9),
    "idle_us": float(span - union_us(idx)),
    "fork_join_generations": sum(1 for i in idx if "init_rows" in names[i] and (i == r0 or "init_rows" not in names[i - 1])),
    "by_kernel_us": {k: round(v, 1) for k, v in collections.Counter({short(names[i]): 0 for i in idx}).items()},
}
for i in idx: right["by_kernel_us"][short(names[i])] = round(right["by_kernel_us"][short(names[i])] + (en[i] - st[i]) / 1e3, 1)
print(f" right-hand part: span {span:.1f} us, {len(steps)} step launches of {right['step_mean_us']:.1f} us, "
      f"{right['steps_running_at_once_mean']:.2f} running at once while any runs, idle {right['idle_us']:.1f} us")
if out_json:
    doc = json.load(open(out_json)) if os.path.isfile(out_json) else {}
    doc[label or args[0]] = right
    json.dump(doc, open(out_json, "w"), indent=1)
