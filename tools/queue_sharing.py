"""Stream -> hardware queue sharing table of one run (ORIP_TRACE_RUN, default 1 = the first timed step of bench.py --warmup 1) inside a rocprofv3
--kernel-trace CSV: per Queue_Id, which lanes' kernels it carried (development aid).  A kernel trace names queues, not streams, so the lanes are told
apart by kernels that only one kind of stream launches: the k_trace launches are one per layer, enqueued dark -> light by orip_contours_prepare, each on
its layer's main stream (layer i = the i-th of them in dispatch order); the other classes say main / side / raster / stage 10 without the layer.  Where
the trace has a Stream_Id column, the distinct ids per queue are listed too.  usage: python tools/queue_sharing.py <dir-or-csv>"""
import csv, glob, os, re, sys
from collections import defaultdict
p = sys.argv[1]
files = [p] if p.endswith(".csv") else sorted(glob.glob(os.path.join(p, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)[-1:]      # the newest run, never a mix
CLASSES = [      # (lane class, kernels only that class of stream launches on the bench path)
    ("raster main", ("k_kmeans_fit", "k_lab_assign", "k_thin_bits04", "k_ccl_bits<IdsBlockRaster>", "k_bits_to_skel_state")),      # (k_ccl_bits<IdsLinear> is stage 08-B's, on the layer streams)
    ("raster side", ("k_chain_ends_bits", "k_chain_build")),
    ("layer main", ("k_trace", "k_greedy_nn_fast", "k_plot_order_wave")),
    ("layer side", ("k_comp_paths_lds", "k_comp_paths_glb", "k_tail_replay", "k_seglen", "k_perim_leaves_seg")),
    ("stage 10", ("k_taps_grid", "k_taps_sequential", "k_stamp_chain", "k_stamp_discs", "k_cut_counts", "k_cut_slots")),
]
LISTED = {k for _, names in CLASSES for k in names}
def short(n):          # the kernel's name without its arguments; without its template arguments too, unless CLASSES lists it with them
    n = re.sub(r"\(anonymous namespace\)::", "", n); n = re.sub(r"^void ", "", n); n = re.sub(r"\(.*", "", n)
    return n if n in LISTED else re.sub(r"<.*", "", n)
rows = []
for f in files:
    with open(f) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r.get("Queue_Id", "?"), int(r.get("Dispatch_Id", 0) or 0), r.get("Stream_Id")))
rows.sort()
starts = [r[0] for r in rows if r[2].startswith("k_kmeans_fit")]
RUN = int(os.environ.get("ORIP_TRACE_RUN", "1")); t0 = starts[RUN]; t_end = starts[RUN + 1] if RUN + 1 < len(starts) else 1 << 62
sel = [r for r in rows if t0 <= r[0] < t_end]
queues = sorted({r[3] for r in sel}, key=lambda q: (len(q), q))
traces = sorted((r for r in sel if r[2] == "k_trace"), key=lambda r: (r[4], r[0]))
layer_of = {id(r): i for i, r in enumerate(traces)}
print(f"run: {(max(r[1] for r in sel) - t0) / 1e6:.1f} ms, {len(sel)} dispatches on {len(queues)} distinct queues, {len(traces)} k_trace launches")
def label_of(on):          # what one stream (or, without stream ids, one queue) carried
    out = []
    for cls, names in CLASSES:
        hit = [r for r in on if r[2] in names or (cls == "raster main" and r[2].startswith("k_kmeans_fit"))]
        if cls == "layer main":
            ls = [layer_of[id(r)] for r in hit if id(r) in layer_of]
            if ls:
                out.append("main of layer" + ("s " if len(ls) != 1 else " ") + ",".join(map(str, ls)))
        elif hit and not (cls == "layer side" and any(o.startswith("main of") for o in out)):      # a main chain runs a few of the side kernels itself
            out.append(cls)
    return " + ".join(out) or "other kernels only"
have_streams = all(r[5] not in (None, "") for r in sel)
mains = defaultdict(list); shared_q = []
for q in queues:
    on = [r for r in sel if r[3] == q]
    busy = sum(e - s for s, e, *_ in on) / 1e6
    mains[q] = [layer_of[id(r)] for r in on if id(r) in layer_of]
    if have_streams:
        sids = sorted({r[5] for r in on}, key=lambda x: (len(x), x))
        what = "; ".join(f"stream {sid}: {label_of([r for r in on if r[5] == sid])} [{sum(e - s for s, e, *x in on if x[-1] == sid) / 1e6:.1f} ms]" for sid in sids)
        if len(sids) > 1:
            shared_q.append(q)
    else:
        what = label_of(on)
    print(f"q{q:>3}: {len(on):5d} dispatches, busy {busy:7.1f} ms | {what}")
shared = {q: ls for q, ls in mains.items() if len(ls) > 1}
print("layer main streams sharing a queue: " + ("; ".join(f"q{q}: layers {','.join(map(str, ls))}" for q, ls in shared.items()) or "none"))
if have_streams:
    print(f"streams with kernels in this run: {len({r[5] for r in sel})}; queues that carry more than one of them: " + (", ".join("q" + q for q in shared_q) or "none"))
