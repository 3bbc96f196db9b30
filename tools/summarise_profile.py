#!/usr/bin/env python
"""Condenses the rocprofv3 outputs of tools/profile_bench.sh into the small files kept under profiles/:
<tag>_kernel_stats.csv (the --stats table) and <tag>_pmc.json (HBM bytes per launch and per kernel:
FETCH_SIZE doubled -- gfx950 tallies 128-byte requests at 64 B, MI355X_MICROARCH.md "HBM" -- plus WRITE_SIZE,
which is exact; L2 hit rate).  The JSON records the hash of the kernel sources it was measured on; bench.py only
quotes `roofline.traffic` from a file whose hash matches the sources it runs.
   summarise_profile.py <tag> [bench.py args]
The same CSV readers condense what the other scripts collect (tools/profile_lib.sh, tools/pmc_diag.sh):
   summarise_profile.py kernels --out-dir D --tag T --note "..." [--flat] KERNEL...   -> D/T_counters_qu30.json
   summarise_profile.py passes --out-dir D --tag T PASS...                            -> counter means per pass and body"""
import csv
import glob
import hashlib
import json
import os
import shutil
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_source_sha():
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "omega_amd", "csrc", "kernels", "*")) +
                   [os.path.join(ROOT, "omega_amd", "csrc", "Makefile")])
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _template_args(s):
    """top-level template arguments of the text after an opening '<'"""
    depth, cur, out = 0, "", []
    for ch in s:
        if ch == "<":
            depth += 1
        elif ch == ">":
            if depth == 0:
                break
            depth -= 1
        elif ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
            continue
        cur += ch
    out.append(cur.strip())
    return out


def short(name):
    """void OMEGA::tileKernel<OMEGA::FusedCell3Body<6, true, false>, ...>(...) -> FusedCell3Body<6, true, false>;
    tileKernel2<A, B, T> (two independent sweeps in one launch) -> A+B"""
    if "tileKernel2<" in name:
        a = _template_args(name[name.index("tileKernel2<") + len("tileKernel2<"):])
        return "+".join(x.replace("OMEGA::", "") for x in a[:2])
    if "tileKernelV<" in name:      # tileKernelV<T, A, B, ...>: any number of independent sweeps in one launch
        a = _template_args(name[name.index("tileKernelV<") + len("tileKernelV<"):])
        return "+".join(x.replace("OMEGA::", "") for x in a[1:])
    if "tileKernel<" in name:
        a = _template_args(name[name.index("tileKernel<") + len("tileKernel<"):])
        return a[0].replace("OMEGA::", "")
    return name.split("(")[0].replace("OMEGA::", "").replace("void ", "").strip()


def counters(dirname, name=short):
    """{name(kernel): {counter: [values]}} of every *counter_collection.csv under dirname"""
    rows = defaultdict(lambda: defaultdict(list))
    for f in glob.glob(os.path.join(dirname, "**", "*counter_collection.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows[name(r["Kernel_Name"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
    return rows


def kernel_stats(dirname):
    """the rows of every *kernel_stats.csv (rocprofv3 --stats) under dirname"""
    rows = []
    for f in glob.glob(os.path.join(dirname, "**", "*kernel_stats.csv"), recursive=True):
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    return rows


def condense_kernels(out_dir, tag, note, kernels, flat=False):
    """What a tools/profile_*.sh keeps of its three profiler steps, as <tag>_counters_qu30.json: per kernel (matched as a
    substring of the full name) the counter means over <tag>_pmc_fetch and <tag>_pmc_write, the HBM bytes per launch
    where both sizes were counted, and the kernel's rows of <tag>_trace's --stats table.  flat: one kernel, its entries
    beside the note."""
    def identity(k):
        return k

    passes = [counters(os.path.join(out_dir, f"{tag}_pmc_{sub}"), identity) for sub in ("fetch", "write")]
    stats = kernel_stats(os.path.join(out_dir, tag + "_trace"))
    res = {"_note": note, "kernels": {}}
    for kern in kernels:
        vals = defaultdict(list)
        for rows in passes:
            for full, by_counter in rows.items():
                if kern in full:
                    for c, v in by_counter.items():
                        vals[c] += v
        mean = {c: sum(v) / len(v) for c, v in vals.items()}
        one = {"launches_sampled": {c: len(v) for c, v in vals.items()}, "counters_mean": mean}
        if "FETCH_SIZE" in mean and "WRITE_SIZE" in mean:
            one["fetch_bytes_per_launch_x2"] = mean["FETCH_SIZE"] * 1024 * 2
            one["write_bytes_per_launch"] = mean["WRITE_SIZE"] * 1024
            one["hbm_bytes_per_launch"] = one["fetch_bytes_per_launch_x2"] + one["write_bytes_per_launch"]
        one["kernel_stats"] = [r for r in stats if kern in r.get("Name", "")]
        res["kernels"][kern] = one
    if flat:
        (one,) = res.pop("kernels").values()
        res.update(one)
    with open(os.path.join(out_dir, tag + "_counters_qu30.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return res


def print_passes(out_dir, tag, passes):
    """tools/pmc_diag.sh: per pass <tag>_<pass> and tile-kernel body, the counter means on one line"""
    for sub in passes:
        for k, v in sorted(counters(os.path.join(out_dir, f"{tag}_{sub}")).items()):
            if "Body" in k:
                print(sub, k[:70], {c: round(sum(x) / len(x), 1) for c, x in v.items()})


def subcommand(argv):
    """kernels --out-dir D --tag T --note "..." [--flat] KERNEL... | passes --out-dir D --tag T PASS..."""
    import argparse
    ap = argparse.ArgumentParser(prog="summarise_profile.py " + argv[0])
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--tag", required=True)
    if argv[0] == "kernels":
        ap.add_argument("--note", default="")
        ap.add_argument("--flat", action="store_true")
    ap.add_argument("names", nargs="+")
    a = ap.parse_args(argv[1:])
    if argv[0] == "kernels":
        condense_kernels(a.out_dir, a.tag, a.note, a.names, a.flat)
    else:
        print_passes(a.out_dir, a.tag, a.names)


def main():
    if sys.argv[1] in ("kernels", "passes"):
        return subcommand(sys.argv[1:])
    tag = sys.argv[1]
    out = os.path.join(ROOT, "gpurun_out")
    fetch, write = counters(os.path.join(out, tag + "_pmc_fetch")), counters(os.path.join(out, tag + "_pmc_write"))
    res = {"_note": "rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum (separate runs) of "
                    "`python3 bench.py --full --steps 8 --warmup 2 --rk4-steps 2 --no-cpu-baseline " + " ".join(sys.argv[2:]) +
                    "`; FETCH_SIZE (KB) x 1024 x 2 (gfx950 half-count of 16-B-per-lane reads) + WRITE_SIZE (KB) x 1024",
           "kernel_source_sha": kernel_source_sha(), "bench_args": sys.argv[2:]}
    total = 0.0
    for k in sorted(set(fetch) | set(write)):
        f, w = fetch.get(k, {}).get("FETCH_SIZE", []), write.get(k, {}).get("WRITE_SIZE", [])
        if not f or not w or "Body" not in k and "Fn" not in k:
            continue
        fb, wb = 2.0 * 1024.0 * sum(f) / len(f), 1024.0 * sum(w) / len(w)
        hit, miss = sum(write[k].get("TCC_HIT_sum", [0])), sum(write[k].get("TCC_MISS_sum", [0]))
        res[k] = {"launches_sampled": len(f), "FETCH_SIZE_KB_raw_mean": sum(f) / len(f),
                  "fetch_bytes_per_launch_gfx950_corrected_x2": fb, "WRITE_SIZE_KB_mean": sum(w) / len(w),
                  "write_bytes_per_launch": wb, "hbm_bytes_per_launch": fb + wb,
                  "L2_hit_rate": hit / (hit + miss) if hit + miss else None}
    with open(os.path.join(out, tag + "_pmc.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    stats = glob.glob(os.path.join(out, tag + "_trace", "**", "*kernel_stats.csv"), recursive=True)
    if stats:
        shutil.copy(stats[0], os.path.join(out, tag + "_kernel_stats.csv"))
    print("[profile] wrote", tag + "_pmc.json", "and", tag + "_kernel_stats.csv" if stats else "(no kernel stats found)")


if __name__ == "__main__":
    main()
