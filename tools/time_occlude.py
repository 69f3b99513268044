"""What --occlude costs (csrc/gcode_occlude.hip), on three drawings in steps: "tiles", --tiles x --tiles closed squares of 40 steps, each painted over the
corner of the one before it and the one above it (every outline is cut twice); "free", --strokes zigzag strokes under --shapes squares that lie beside them
(nothing to hide: the price of the option when the boxes refuse everything); "comb", one stroke of --segments segments across a comb of --teeth teeth and
under a polygon of --edges edges: many events on a segment, many edges in a shape.  Per drawing: the orip_gcode_occlude call on the uploaded strokes and
rings by the host clock (the call ends in a stream synchronisation; the uploads and its three read-backs are inside it, the fetches are not), median of
--reps after one warm-up call; its phases (orip_prof_get, in runs of their own: every timed scope ends in an event wait); the stats; the same clock around
orip_gcode_dedup on the same strokes; and, up to --check-segments segments, the comparison with the sequential definition (tests/occlude_double.py).
--lib FILE loads another build of the library, so that two builds can be timed from one tree.
usage: python tools/time_occlude.py [--tiles K] [--strokes N] [--shapes N] [--teeth N] [--edges N] [--segments N] [--reps K] [--lib FILE] [--out FILE.json]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SIDE = 40
PHASES = ("oc_cand", "oc_count", "oc_pieces", "oc_compact", "oc_emit")


def arrays(strokes, levels, rings, ring_levels):
    off = lambda ls: np.concatenate([[0], np.cumsum([len(p) for p in ls])]).astype(np.int64)
    cat = lambda ls: np.concatenate([np.asarray(p, np.int32).reshape(-1, 2) for p in ls]) if ls else np.zeros((0, 2), np.int32)
    return off(strokes), cat(strokes), np.asarray(levels, np.int32), off(rings), cat(rings), np.asarray(ring_levels, np.int32)


def tiles(k):
    sq = np.array([(0, 0), (SIDE, 0), (SIDE, SIDE), (0, SIDE)], np.int32)
    at = [sq + (100 + 30 * i, 100 + 30 * j) for j in range(k) for i in range(k)]
    return arrays([np.concatenate([r, r[:1]]) for r in at], list(range(len(at))), at, list(range(len(at))))


def free(n, shapes, seed=5):
    rng = np.random.default_rng(seed)
    lists = []
    for i in range(n):
        x = np.cumsum(rng.integers(1, 9, int(rng.integers(2, 9)))) + int(rng.integers(0, 5000))
        lists.append(np.stack([x, 10 * i + 7 * (np.arange(len(x)) & 1)], 1))
    sq = np.array([(0, 0), (SIDE, 0), (SIDE, SIDE), (0, SIDE)], np.int32)
    rings = [sq + (6000 + 50 * (s % 100), 50 * (s // 100)) for s in range(shapes)]
    return arrays(lists, [0] * n, rings, list(range(1, shapes + 1)))


def comb(teeth, edges, segments):
    ring = [(10, 0), (10 + 4 * teeth, 0)]
    for k in reversed(range(teeth)):
        x = 10 + 4 * k
        ring += [(x + 4, 5), (x + 3, 5), (x + 3, 2000), (x + 1, 2000), (x + 1, 5)]
    ring += [(10, 5)]
    r, c = 900, 1000
    poly = [(c + round(r * math.cos(2 * math.pi * k / edges)), c + round(r * math.sin(2 * math.pi * k / edges))) for k in range(edges)]
    w = 4 * teeth + 20
    stroke = [((w if j & 1 else 0), 10 + 3 * j) for j in range(segments + 1)]
    return arrays([stroke], [0], [ring, poly], [1, 2])


def clock(fn, reps):
    t = []
    for rep in range(reps + 1):
        t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
        if rep:
            t.append(t1 - t0)
    return {"s_median": float(np.median(t)), "s_min_max": [float(min(t)), float(max(t))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=100)
    ap.add_argument("--strokes", type=int, default=10000)
    ap.add_argument("--shapes", type=int, default=1000)
    ap.add_argument("--teeth", type=int, default=1000)
    ap.add_argument("--edges", type=int, default=10000)
    ap.add_argument("--segments", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-segments", type=int, default=3000)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlude_times.json"))
    a = ap.parse_args()
    from orip import lib
    if a.lib:
        lib.LIB_PATH = os.path.abspath(a.lib)
    from orip.device import Device
    import occlude_double as OD
    inputs = {"tiles": tiles(a.tiles), "free": free(a.strokes, a.shapes), "comb": comb(a.teeth, a.edges, a.segments)}
    res = {k: getattr(a, k) for k in ("tiles", "strokes", "shapes", "teeth", "edges", "segments", "reps")}
    res.update(side_steps=SIDE, lib=a.lib, inputs={})
    dev = Device(0)
    try:
        for name, arr in inputs.items():
            off, pts, level, r_off, r_pts, r_level = [np.ascontiguousarray(v) for v in arr]
            n, m = len(off) - 1, len(r_level)
            st10, st9 = np.zeros(10, np.int64), np.zeros(9, np.int64)
            call = lambda: dev._ck(dev.L.orip_gcode_occlude(dev.h, off.ctypes.data, pts.ctypes.data, level.ctypes.data, n, r_off.ctypes.data, r_pts.ctypes.data,
                                                            r_level.ctypes.data, m, st10.ctypes.data))
            r = {"strokes": n, "points": len(pts), "rings": m, "ring_points": len(r_pts)}
            r["occlude"] = clock(call, a.reps)
            r["stats"] = {k: int(v) for k, v in zip(lib.OCCLUDE_STATS, st10)}
            kern = {k: [] for k in PHASES}
            for rep in range(a.reps):
                dev.prof_reset(); dev.prof_enable(True); call(); dev.prof_enable(False)
                for k in kern:
                    kern[k].append(dev.prof_get(k)[0] * 1e-3)
            r["phases_s_median"] = {k: float(np.median(v)) for k, v in kern.items()}
            r["dedup"] = clock(lambda: dev._ck(dev.L.orip_gcode_dedup(dev.h, off.ctypes.data, pts.ctypes.data, None, n, 1, st9.ctypes.data)), a.reps)
            if len(pts) - n <= a.check_segments and (name != "comb" or a.teeth * a.segments <= 2000):      # the double tests every stretch against every edge
                got = dev.gcode_occlude(*arr)
                want = OD.occlude_numpy(*arr)
                r["equals_sequential_definition"] = bool(all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3])) and got[3] == want[3])
            res["inputs"][name] = r
    finally:
        dev.close()
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
