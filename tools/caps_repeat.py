"""How often stage 08-A stamps the same capsule again within R consecutive samples, on the CPU with the oracle alone (development aid; the motivation of
the set in LDS of k_caps_insert).

The top-left CROP x CROP pixels of the bench image (synth_image(SIZE, SIZE, K)) go through run_pipeline(upto=7); per layer the polylines are resampled in
descending-perimeter order (08:53-64; split_small_taps08 is NOT applied, so short polylines count too: the figures are approximate), the capsule key of a
sample is the unordered pair of its rounded pixel and its predecessor's.  Per layer and R: capsules / sum over contiguous ranges of R samples of the
distinct keys in the range -- one probe of the table in that many samples is left when a workgroup remembers the keys of its range.

usage: python tools/caps_repeat.py [CROP [SIZE [K [R ...]]]]          default: 1024 4096 8 1024 8192 65536"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT)
import numpy as np
from oracle import oracle as O
from orip.synth import synth_image, layer_names

a = [int(x) for x in sys.argv[1:]]
crop = a[0] if len(a) > 0 else 1024; size = a[1] if len(a) > 1 else 4096; K = a[2] if len(a) > 2 else 8
Rs = a[3:] or [1024, 8192, 65536]
names = layer_names(K)
cfg = dict(O.DEFAULTS, color_names=names)
img = np.ascontiguousarray(synth_image(size, size, K)[:crop, :crop])
res = O.run_pipeline(img, cfg, upto=7)
step = max(1.0, float(cfg["dedup_sample_step"]))
print("| layer | samples | " + " | ".join("R = %d" % r for r in Rs) + " | whole layer |")
print("|---|---|" + "---|" * (len(Rs) + 1))
for n in names:
    polys = sorted(res["sorted"][n], key=lambda p: -O.poly_perimeter(p))          # (stable: equal perimeters keep their order)
    keys = []
    for p in polys:
        q = np.asarray(p).reshape(-1, 2); m = len(q)
        if m >= 2 and (q[0] == q[m - 1]).all():
            m -= 1
        if m < 2:
            continue
        S, _ = O.resample_arclen(q[:m].astype(np.float32), False, step)
        if len(S) < 2:
            continue
        r = np.rint(np.asarray(S, np.float64)).astype(np.int64)
        pt = (r[:, 0] << 14) | r[:, 1]
        lo = np.minimum(pt[1:], pt[:-1]); hi = np.maximum(pt[1:], pt[:-1])
        keys.append((lo << 28) | hi)
    if not keys:
        continue
    k = np.concatenate(keys); total = len(k)
    cols = []
    for R in Rs + [total]:
        distinct = sum(len(np.unique(k[i:i + R])) for i in range(0, total, R))
        cols.append("%.1f" % (total / distinct))
    print("| `%s` | %d | " % (n, total) + " | ".join(cols) + " |")
