"""Per timed step of a `rocprofv3 --kernel-trace --output-format csv` run of bench.py: the time from the step's first kernel
to the start of its first k_gate16 (layer 0's step 0), and the kernels of all streams started in between (the fill kernels
of hipMemsetAsync included).  A step ends with its k_head.  Prints median and spread over the last <timed steps> steps and
the kernel list of the last one (profiles/forward_setup_*_setup_chain.txt).
usage: setup_chain.py <kernel_trace.csv> <timed steps>"""
import csv, re, statistics, sys
rows = list(csv.DictReader(open(sys.argv[1])))
steps_timed = int(sys.argv[2])
ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows))
steps, cur = [], []
for k in ks:
    cur.append(k)
    if re.search(r"\bk_head\b", k[2]):
        steps.append(cur); cur = []
res = []
for s in steps:
    names = [k[2] for k in s]
    gi = next((i for i, n in enumerate(names) if "k_gate16" in n), None)
    if gi is None or not any("k_fuse_heads" in n for n in names[:gi]):
        continue
    res.append(((s[gi][0] - s[0][0]) / 1e3, gi, names[:gi], names[gi]))
res = res[-steps_timed:]
us = [r[0] for r in res]; n = [r[1] for r in res]
print("steps %d: first kernel -> first k_gate16 start: median %.1f us, min %.1f, max %.1f, p10 %.1f, p90 %.1f; kernels before it (all streams): median %d (min %d max %d)" % (
    len(res), statistics.median(us), min(us), max(us), sorted(us)[len(us) // 10], sorted(us)[-1 - len(us) // 10], statistics.median(n), min(n), max(n)))
print("gate kernel:", res[-1][3][:120])
for nm in res[-1][2]:
    print("   ", nm[:100])
