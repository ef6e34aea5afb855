"""Per-launch table of a rocprofv3 --kernel-trace database: kernels grouped by (name, blocks per launch) with launches per UNet
forward, average and standard deviation of the launch duration and time per forward -- the form of profiles/r07_ff_proj_fold_trace.txt
and profiles/r08_wstream_epi_trace.txt (two launches of one instantiation with different grids are different rows).

    python tools/launch_table.py trace.db [substring of the kernel name ...]      (default: gemm, splitk, ff_chain)"""
import math
import re
import sqlite3
import sys


def load(path):
    cur = sqlite3.connect(path).cursor()
    tabs = [r[0] for r in cur.execute("select name from sqlite_master where type in ('view','table')")]
    t = ([x for x in tabs if x == "kernels"] or [x for x in tabs if "kernel_dispatch" in x])[0]
    cols = [c[1] for c in cur.execute("pragma table_info('%s')" % t)]
    ci = {c: i for i, c in enumerate(cols)}
    name_c = "name" if "name" in ci else [c for c in cols if "name" in c][0]

    def prod(r, stem):
        v = 1
        for ax in "xyz":
            v *= max(int(r[ci["%s_%s" % (stem, ax)]]), 1)
        return v

    rows = []
    for r in cur.execute("select * from %s" % t):
        if "grid_x" in ci:
            wg = prod(r, "workgroup") if "workgroup_x" in ci else 1
            blocks = prod(r, "grid") // wg
        elif "grid_size" in ci:
            blocks = int(r[ci["grid_size"]]) // max(int(r[ci["workgroup_size"]]) if "workgroup_size" in ci else 1, 1)
        else:
            blocks = 0
        rows.append((re.sub(r"^void ", "", r[ci[name_c]]), blocks, (r[ci["end"]] - r[ci["start"]]) / 1e3))
    return rows


def main():
    rows = load(sys.argv[1])
    want = sys.argv[2:] or ["gemm", "splitk", "ff_chain"]
    forwards = sum(1 for n, _, _ in rows if "nhwc_to_nchw_kernel" in n) or 1     # the eps transpose that ends a forward
    total = sum(d for _, _, d in rows)
    print("%d forwards, %.1f us of kernel time per forward, %.0f dispatches per forward" % (forwards, total / forwards, len(rows) / forwards))
    agg = {}
    for n, b, d in rows:
        if any(w in n for w in want):
            agg.setdefault((n, b), []).append(d)
    for (n, b), ds in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        mean = sum(ds) / len(ds)
        std = math.sqrt(sum((d - mean) ** 2 for d in ds) / max(len(ds) - 1, 1))
        if sum(ds) / forwards < 5.0:
            continue
        print("%-100s blocks=%-6d per_fwd=%6.2f avg_us=%8.2f std_us=%6.2f us_per_fwd=%9.1f" % (
            n[:100], b, len(ds) / forwards, mean, std, sum(ds) / forwards))


if __name__ == "__main__":
    main()
