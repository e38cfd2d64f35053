"""launch_diff.py -- the kernel launches of two rocprofv3 kernel traces side by side (developer tool).

Per (kernel, grid) the launch counts of both runs, and whether each queue's launch order is the same; only the
launches after the set-up (the context's warm-up calls, the files' fills, torch's edit of the bases) are compared.
usage: python launch_diff.py PARENT_TRACE_DIR NEW_TRACE_DIR > out.txt
(the -d directories of two `rocprofv3 --kernel-trace --output-format csv` runs of bench.py)
"""
import collections
import csv
import glob
import re
import sys


def load(d):
    rows = []
    for p in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        with open(p, newline="") as f:
            for r in csv.DictReader(f):
                name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("rsh::", "")
                grid = "x".join(r[k] for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z") if k in r)
                rows.append((int(r["Start_Timestamp"]), r.get("Queue_Id", "?"), name, grid))
    rows.sort()
    last = max(i for i, r in enumerate(rows) if r[2].startswith("fill_words") or "at::native" in r[2])
    return rows[last + 1:]


def per_queue(rows):
    """Each queue's (kernel, grid) sequence; queue ids differ between processes, so queues in order of first use."""
    q = collections.OrderedDict()
    for _, qi, n, g in rows:
        q.setdefault(qi, []).append((n, g))
    return list(q.values())


def main():
    a, b = load(sys.argv[1]), load(sys.argv[2])
    ca = collections.Counter((n, g) for _, _, n, g in a)
    cb = collections.Counter((n, g) for _, _, n, g in b)
    print(f"launches: parent {len(a)}, new {len(b)}; (kernel, grid) counts {'equal' if ca == cb else 'DIFFER'}")
    print(f"{'kernel':60s} {'grid':>16s} {'parent':>7s} {'new':>7s}")
    for k in sorted(set(ca) | set(cb)):
        print(f"{k[0][:60]:60s} {k[1]:>16s} {ca[k]:7d} {cb[k]:7d}{'' if ca[k] == cb[k] else '   <-- differs'}")
    qa, qb = per_queue(a), per_queue(b)
    print(f"queues: parent {len(qa)}, new {len(qb)}")
    for i, (x, y) in enumerate(zip(qa, qb)):
        print(f"queue {i}: parent {len(x)} launches, new {len(y)}: order {'equal' if x == y else 'DIFFERS'}")
        diff = next((j for j, (u, v) in enumerate(zip(x, y)) if u != v), None)
        if diff is not None:
            print(f"   first difference at launch {diff}: parent {x[diff]}, new {y[diff]}")


if __name__ == "__main__":
    main()
