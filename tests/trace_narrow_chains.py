"""Developer tool: from a rocprofv3 kernel trace of bench.py (a directory or a kernel_trace.csv), the narrowphase kernels over the
last N steps: busy time per step and queue of each, the wall span of the two chains (k_gjk<0> -> k_epa<0>; k_narrow<0>, k_narrow<1>)
from the first start to the later end, how long a kernel of each chain ran at the same time, the gaps in front of and behind the
chains, and the last step's start and end stamps (profiles/narrow_overlap.txt)."""
import csv, sys, glob, os, collections
path, steps = sys.argv[1], int(sys.argv[2])
files = [path] if os.path.isfile(path) else glob.glob(path + "/**/*kernel_trace.csv", recursive=True)
rows = []
for f in files:
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "?")))
rows.sort()
# a step = from one k_build_colliders to the next
starts = [i for i, r in enumerate(rows) if "k_build_colliders" in r[2]][-(steps + 1):]
NAMES = ["k_classify", "k_bucket_offsets", "k_gjk<0>", "k_narrow<0>", "k_narrow<1>", "k_epa<0>"]
busy, queues = collections.defaultdict(float), collections.defaultdict(set)
all_busy = 0
spans, both, fork, join = [], [], [], []
for a, b in zip(starts[:-1], starts[1:]):
    ev = {}
    for s, e, name, q in rows[a:b]:
        all_busy += e - s
        for k in NAMES:
            if k in name:
                busy[k] += e - s
                queues[k].add(q)
                ev[k] = (s, e)    # a step that runs its narrowphase twice: the launch that stands
    if all(k in ev for k in NAMES[1:]):
        off, g, cl, bx, ep = (ev[k] for k in NAMES[1:])
        first, last = min(g[0], cl[0]), max(ep[1], bx[1])
        spans.append(last - first)
        both.append(sum(max(0, min(x[1], y[1]) - max(x[0], y[0])) for x in (g, ep) for y in (cl, bx)))
        fork.append((first - off[1], cl[0] - off[1], g[0] - off[1]))
        later = [s for s, e, name, q in rows[a:b] if s >= last]
        join.append(min(later) - last if later else 0)
n = len(starts) - 1
print("last %d steps: step span %.1f us/step, all kernels busy %.1f us/step" % (n, (rows[starts[-1]][0] - rows[starts[0]][0]) / n / 1e3, all_busy / n / 1e3))
for k in NAMES:
    print("  %-18s %8.1f us/step   queue %s" % (k, busy[k] / n / 1e3, ",".join(sorted(queues[k]))))
if spans:
    m = len(spans)
    print("  chains, first start to later end: %.1f us/step (min %.1f, max %.1f)" % (sum(spans) / m / 1e3, min(spans) / 1e3, max(spans) / 1e3))
    print("  a kernel of each chain running at once: %.1f us/step" % (sum(both) / m / 1e3))
    print("  k_bucket_offsets end -> first chain kernel +%.1f us, k_narrow<0> +%.1f us, k_gjk<0> +%.1f us" % tuple(sum(f[i] for f in fork) / m / 1e3 for i in range(3)))
    print("  later chain end -> next kernel +%.1f us" % (sum(join) / m / 1e3))
    t0 = rows[starts[-2]][0]
    print("  last step (start, end in us from the step's start, queue):")
    for s, e, name, q in rows[starts[-2]:starts[-1]]:
        if any(k in name for k in NAMES):
            print("    %-32s %8.1f %8.1f  q%s" % (name.split("(")[0][-32:], (s - t0) / 1e3, (e - t0) / 1e3, q))
