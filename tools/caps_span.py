"""Stage 08-A4 in a kernel trace (development aid; profiles/capsset_*_span.txt are its output).
usage: python tools/caps_span.py <kernel_trace.csv of rocprofv3 --kernel-trace --output-format csv over bench.py (8 layers)>
Prints the launch count of every kernel, k_caps_insert's total and longest launch, and, on the queues of the two longest k_caps_insert launches of the last
step (the heavy layers), the span from the start of k_samples to the end of k_accept_brute with the kernels in it; on the same queues the wait for the tail
replay (end of k_caps_stamp_bits -> start of k_accept_pre) with that layer's k_tail_replay, and the k_comp_keys launch behind the span; last, the totals of
k_comp_keys and k_tail_replay (profiles/tailstop_*_span.txt)."""
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
    # the wait for the tail replay: no host read or dispatch lies between k_caps_stamp_bits and k_accept_pre, so a gap there is the wait for the side stream
    in_span = [r for r in rows if r[3] == q and s[1] <= r[1] and r[2] <= e[2]]
    stamp = max((r for r in in_span if "k_caps_stamp_bits" in r[0]), key=lambda r: r[2])
    pre = min((r for r in in_span if "k_accept_pre" in r[0] and r[1] >= stamp[2]), key=lambda r: r[1])
    par = max((r for r in in_span if "k_tail_par" in r[0]), key=lambda r: r[2])
    # the layer's replay runs on another queue.  Its side stream waits for exactly this k_tail_par and k_accept_pre waits for its end, so it starts behind
    # par's end and ends before pre's start.  Other layers' launches may do so too: the one on the queue behind this one is taken (a lane's main and side
    # stream sit on a queue pair), else the first to start
    cand = [r for r in rows if "k_tail_replay" in r[0] and r[1] >= par[2] and r[2] <= pre[1]]
    pair = [r for r in cand if q.isdigit() and r[3] == str(int(q) + 1)]
    rep = min(pair or cand, key=lambda r: r[1])
    print("   k_caps_stamp_bits end -> k_accept_pre start %.3f ms; k_tail_replay (queue %s) %.3f ms, ends %.3f ms behind k_tail_par and %.3f ms before k_accept_pre starts"
          % ((pre[1] - stamp[2]) / 1e6, rep[3], (rep[2] - rep[1]) / 1e6, (rep[2] - par[2]) / 1e6, (pre[1] - rep[2]) / 1e6))
    ck = [r for r in rows if "k_comp_keys" in r[0] and r[3] == q and r[1] >= e[2]]
    if ck: print("   k_comp_keys behind it on this queue %.3f ms" % ((ck[0][2] - ck[0][1]) / 1e6))
keys = [(r[2] - r[1]) / 1e6 for r in rows if "k_comp_keys" in r[0]]
print("k_comp_keys launches %d total %.3f ms longest %.3f ms" % (len(keys), sum(keys), max(keys)))
rep = [(r[2] - r[1]) / 1e6 for r in rows if "k_tail_replay" in r[0]]
print("k_tail_replay launches %d total %.3f ms longest %.3f ms" % (len(rep), sum(rep), max(rep)))
