"""Table of a -Rpass-analysis=kernel-resource-usage report: python tools/resource_table.py REPORT [REPORT2] [name-filter]

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -I include -I flash_viterbi_amd/csrc \
        --cuda-device-only -Rpass-analysis=kernel-resource-usage -c flash_viterbi_amd/csrc/fv_full.hip -o /dev/null 2> REPORT

One row per kernel whose demangled name contains the filter (default trellis_step_u16): VGPRs, SGPRs, scratch bytes per lane,
spilled VGPRs, waves per SIMD.  With two reports: the first beside the second ("before -> after"; "-" where a kernel is in one
report only)."""
import re
import subprocess
import sys

KEYS = (("VGPRs", "VGPRs"), ("TotalSGPRs", "SGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("VGPRs Spill", "spill"), ("Occupancy [waves/SIMD]", "waves"))


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
        if m and name:
            out[name][m.group(1)] = m.group(2)
    return out


def demangle(names):
    p = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True)
    nice = p.stdout.split("\n") if p.returncode == 0 else list(names)
    # (a last template argument that is a defaulted `true` is dropped: the same kernel in a report from before it existed)
    return {n: re.sub(r"^(\w+<(?:[^,<>]+, ){4})true>$", lambda m: m.group(1)[:-2] + ">", re.sub(r"^void fvk::|\(fvk::StepArgs<.*$", "", d))
            for n, d in zip(names, nice)}


if __name__ == "__main__":
    files = [a for a in sys.argv[1:] if "." in a or "/" in a][:2]
    filt = next((a for a in sys.argv[1:] if a not in files), "trellis_step_u16")
    reports = [parse(f) for f in files]
    nice = demangle(sorted({n for r in reports for n in r if filt in n}))
    reports = [{nice[n]: v for n, v in r.items() if n in nice} for r in reports]
    names = sorted(set(nice.values()))
    print("| kernel | " + " | ".join(k for _, k in KEYS) + " |")
    print("|---|" + "---|" * len(KEYS))
    for n in names:
        cells = []
        for key, _ in KEYS:
            vals = [r.get(n, {}).get(key, "-") for r in reports]
            cells.append(vals[0] if len(set(vals)) == 1 else " -> ".join(vals))
        print(f"| `{n}` | " + " | ".join(cells) + " |")
