"""Inputs for the capsule de-duplication of stage 08-A (k_caps_insert: a workgroup owns a range of samples and keeps the capsule keys it has seen in LDS),
shared by test_gpu_stage08_capsules.py and its no-GPU companion test_oracle_capsule_cases.py.

What has to be told apart.  The capsule table must hold, per distinct capsule, the SMALLEST sample index that stamps it.  A sample is dropped when its
pixel was stamped before its own pops (the canvas, shared by the polylines of a layer) or when a popped sample of its own polyline lies within the
collision radius (the point hash, per polyline).  A lap that repeats an earlier lap sample for sample is dropped by the hash whatever the table holds, so
such laps say nothing about the table.  The rings here are therefore walked at a step of 4 px with a perimeter of 4k + 2 px (axis-parallel, integer
corners, width + height odd) and a collision radius of 1.4 px (capsule radius 1 px):

  lap 1, 3, 5 ...   samples at arc 0, 4, 8 ... of the ring: the same rounded pixels, the same capsule keys, lap after lap
  lap 2, 4, 6 ...   samples 2 px further on: midway between the samples of the odd laps, 2 px from the nearest of them -- outside the hash's radius, on
                    the odd laps' capsules

The perimeter is longer than the tail (120 px), so lap 1 has been popped when lap 2 passes: lap 2 is dropped only because lap 1's capsules carry lap 1's
sample indices.  A table that kept the index of lap 3 for a capsule of lap 1 would stamp it after lap 2 has been decided, and lap 2 would stay."""
import functools
import math

import numpy as np

from oracle import oracle as O

STEP = 4
CFG = dict(O.DEFAULTS, pixels_per_mm=6, dedup_sample_step=STEP, collision_radius_intra_px=1.4, ignore_tail_points_intra=120)      # canvas 1260 x 1782
CHUNK = 1024


def P(a):
    return np.asarray(a, np.int32).reshape(-1, 1, 2)


def ring_path(x0, y0, w, h, laps, drop=1):
    """`laps` times round the rectangle from its corner (x0, y0), without the last `drop` edges (so the path does not end on its first point and is a little
    shorter per edge dropped)"""
    assert (w + h) % 2 == 1 and 2 * (w + h) > CFG["ignore_tail_points_intra"]
    c = [[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]]
    pts = (c * laps + [c[0]])[:4 * laps + 1 - drop]
    return P(pts)


def path_len(p):
    a = np.asarray(p, np.int64).reshape(-1, 2)
    return int(np.abs(a[1:] - a[:-1]).sum())           # axis-parallel


def n_samples(p):
    return math.ceil(path_len(p) / STEP)


def lead_path(n, x0=40, y0=60, width=1100, pitch=14):
    """an open path of exactly n samples (rows left to right and back, 4n px long), above the rings that follow it"""
    total = STEP * n
    pts = [[x0, y0]]; left = total; r = 0
    while left > 0:
        run = min(width, left); sgn = -1 if r & 1 else 1
        pts.append([pts[-1][0] + sgn * run, pts[-1][1]]); left -= run
        if left > 0:
            down = min(pitch, left); pts.append([pts[-1][0], pts[-1][1] + down]); left -= down
        r += 1
    return P(pts)


# name -> (polylines in processing order (perimeter, descending), samples per polyline)
RING_S = (60, 1000, 400, 201)           # 300.5 samples a lap
RING_A = (60, 1000, 500, 301)           # 400.5 samples a lap: shape 1
RING_B = (60, 40, 1100, 1701)           # 1400.5 samples a lap: shape 2


def _cases():
    c = {}
    c["ring400_3laps"] = [ring_path(*RING_A, 3)]                       # 1. lap 3 starts at sample 801: the repeats in the chunk of their first occurrence
    c["ring1400_3laps"] = [ring_path(*RING_B, 3)]                      # 2. lap 3 starts at sample 2801: a later chunk
    c["ring1400_50laps"] = [ring_path(*RING_B, 50)]                    # 3. 69 600 samples: repeats of lap 1 beyond 65 536 samples
    for n in (1023, 1024, 1025):                                       # 4. the ring starts anywhere in a chunk ...
        c["lead%d_ring300" % n] = [lead_path(n), ring_path(*RING_S, 3)]
    for R in (8192, 16384):                                            #    ... and in a range
        for n in (R - 1, R, R + 1):
            c["lead%d_ring400" % n] = [lead_path(n), ring_path(*RING_A, 3)]
    c["two_over_one_ring"] = [ring_path(*RING_B, 3), ring_path(*RING_B, 3, drop=2)]      # 5. the second polyline repeats the first one's capsules
    c["ring_leaves_canvas"] = [ring_path(-150, 100, 500, 301, 3)]                       # 6. x from -150: samples off the canvas, capsules across the gap
    return c


CASES = _cases()
LAPS = {"ring1400_50laps": 50}


def ring_of(name):
    """(index of the first lapped polyline, its ring's samples per lap (x.5))"""
    polys = CASES[name]
    i = 0 if len(polys) == 1 or name == "two_over_one_ring" else 1
    a = np.asarray(polys[i]).reshape(-1, 2)
    return i, 2 * (abs(int(a[1][0] - a[0][0])) + abs(int(a[2][1] - a[1][1]))) / STEP


@functools.lru_cache(maxsize=None)
def samples(name):
    """per polyline, the oracle's resampled positions (08:53-64 behind the split of 08:127)"""
    prm = O.derived08(CFG); out = []
    for p in CASES[name]:
        kept, _ = O.split_small_taps08([p], prm)
        assert len(kept) == 1
        a = np.asarray(kept[0]).reshape(-1, 2)
        assert not (a[0] == a[-1]).all()
        S, ps = O.resample_arclen(a.astype(np.float32), False, float(STEP))
        assert not ps
        out.append(np.asarray(S, np.float64))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's stage 08 of the case: computed once, shared, never changed"""
    return O.stage08_layer(CASES[name], O.derived08(CFG))


def capsule_keys(name):
    """global sample index -> capsule key (None: no capsule), as stage 08-A forms them: rounded pixels of a sample and of the previous in-canvas sample of
    its polyline, unordered"""
    W, H = O.canvas_size(CFG); keys = []
    for S in samples(name):
        r = np.rint(S).astype(np.int64); last = None
        for x, y in r:
            if not (0 <= x < W and 0 <= y < H):
                keys.append(None); continue
            cur = (int(x), int(y))
            keys.append(None if last is None else (min(last, cur), max(last, cur)))
            last = cur
    return keys


def first_and_repeats(name):
    """{key: [sample indices, ascending]} for the keys that occur more than once"""
    d = {}
    for g, k in enumerate(capsule_keys(name)):
        if k is not None:
            d.setdefault(k, []).append(g)
    return {k: v for k, v in d.items() if len(v) > 1}
