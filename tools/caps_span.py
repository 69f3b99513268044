"""Stage 08-A4 in a kernel trace (development aid; profiles/capsset_*_span.txt are its output).
usage: python tools/caps_span.py <kernel_trace.csv of rocprofv3 --kernel-trace --output-format csv over bench.py (8 layers)>
Prints the launch count of every kernel, k_caps_insert's total and longest launch, and, on the queues of the two longest k_caps_insert launches of the last
step (the heavy layers), the span from the start of k_samples to the end of k_accept_brute with the kernels in it."""
import csv, re, sys
from collections import defaultdict
rows = []
with open(sys.argv[1]) as fh:
    for r in csv.DictReader(fh):
        k = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"]); k = re.sub(r"\(.*", "", k).replace("void ", "")
        rows.append((k, int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"]))
rows.sort(key=lambda r: r[1])
cnt = defaultdict(int)
for r in rows: cnt[r[0]] += 1
print("kernels", len(cnt), "launches", len(rows))
for k in sorted(cnt): print("COUNT", k, cnt[k])
caps = [r for r in rows if "k_caps_insert" in r[0]]
d = [(r[2] - r[1]) / 1e6 for r in caps]
print("k_caps_insert launches %d total %.3f ms longest %.3f ms" % (len(caps), sum(d), max(d)))
per_step = 8
last = caps[-per_step:]
print("last step k_caps_insert ms:", ["%.3f" % ((r[2] - r[1]) / 1e6) for r in last])
heavy = sorted(last, key=lambda r: r[1] - r[2])[:2]
for h in heavy:
    q = h[3]
    s = max((r for r in rows if "k_samples<" in r[0] and r[3] == q and r[1] < h[1]), key=lambda r: r[1])
    e = min((r for r in rows if "k_accept_brute" in r[0] and r[3] == q and r[2] > h[2]), key=lambda r: r[2])
    print("queue %s: k_caps_insert %.3f ms; k_samples start -> k_accept_brute end %.3f ms" % (q, (h[2] - h[1]) / 1e6, (e[2] - s[1]) / 1e6))
    for r in rows:
        if r[3] == q and s[1] <= r[1] and r[2] <= e[2]:
            print("   %-40s +%.3f  %.3f ms" % (r[0][:40], (r[1] - s[1]) / 1e6, (r[2] - r[1]) / 1e6))
