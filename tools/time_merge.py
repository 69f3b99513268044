"""What --merge-paths costs and saves (csrc/gcode_merge.hip), on the input it is for: a curve of --points points on an A4 sheet exploded into two-point
strokes, the file order shuffled, every other stroke flipped.  The whole tool (orip.gcode.build_stream_from_gcode on the paths in mm, --allow-reverse) runs
without and with the option; per step the host clock of its lap (each ends in a stream synchronisation), medians of --reps after one warm-up run; the
pen-down commands of both streams as the stage-14 decoder counts them; and the merge call alone with its kernels' times (orip_prof_get).  At --check-size
the merge is compared with the sequential definition (tests/merge_double.py).
usage: python tools/time_merge.py [--points N] [--reps K] [--check-size N] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def exploded_curve(points, seed=7):
    """(off, pts_mm): a 31:29 Lissajous curve through `points` points inside the A4 margins, as points - 1 two-point strokes, shuffled, about half flipped"""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 2.0 * np.pi, points)
    P = np.stack([105.0 + 90.0 * np.sin(31.0 * t + 0.5), 148.5 + 130.0 * np.sin(29.0 * t)], 1)     # about 18 m of line: 7 steps a stroke at 10^5 points
    seg = np.stack([P[:-1], P[1:]], 1)[rng.permutation(points - 1)]
    flip = rng.random(points - 1) < 0.5
    seg[flip] = seg[flip][:, ::-1]
    return np.arange(points) * 2, seg.reshape(-1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check-size", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip.device import Device
    from orip import gcode as GC, stream_preview as SP
    import merge_double as MD
    off, pts = exploded_curve(a.points)
    res = {"points": a.points, "strokes": a.points - 1}
    dev = Device(0)
    try:
        for name, merge in (("without", False), ("with", True)):
            o = GC.GcodeOptions(allow_reverse=True, merge_paths=merge)
            laps, whole = [], []
            for rep in range(a.reps + 1):
                tm = {}
                t0 = time.perf_counter(); data, info = GC.build_stream_from_gcode((off, pts), o, dev, timings=tm); t1 = time.perf_counter()
                if rep:                                                       # the first run loads code objects and grows buffers
                    laps.append(tm); whole.append(t1 - t0)
            W, H = info["target"]
            st = SP.preview(dev, data, W, H, 600, 848, invert_y=True)[1]
            res[name] = {"whole_s_median": float(np.median(whole)), "laps_s_median": {k: float(np.median([l[k] for l in laps])) for k in laps[0]}, "reps": a.reps,
                         "paths": info["paths"], "pen_down_commands": st["pen_down_segments"], "steps_total": st["steps_total"], "bytes": len(data)}
            if merge:
                res[name]["merge"] = info["merge"]
        # the merge call alone, on the resident polylines of a fresh conversion
        W, H = GC.target_size(GC.GcodeOptions())
        m = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=40.0, W=W, H=H, invert_y=0)
        call, kern = [], {"k_mg_insert": [], "k_mg_jump": [], "k_mg_emit": []}
        for rep in range(a.reps + 1):
            s_off, _ = dev.gcode_to_steps(off, pts, m)
            n = len(s_off) - 1
            dev.prof_reset(); dev.prof_enable(rep > 0)
            t0 = time.perf_counter(); out = dev.gcode_merge(None, None, None, 1, True, n=n); t1 = time.perf_counter()
            dev.prof_enable(False)
            if rep:
                call.append(t1 - t0)
                for k in kern:
                    kern[k].append(dev.prof_get(k)[0] * 1e-3)
        res["merge_call"] = {"paths_in": n, "call_with_fetch_s_median": float(np.median(call)), "kernels_s_median": {k: float(np.median(v)) for k, v in kern.items()},
                             "note": "with the profile on, every timed kernel is followed by an event wait", "stats": out[5]}
        if a.check_size:
            k = min(a.points, a.check_size)
            c_off, c_pts = dev.gcode_to_steps(*exploded_curve(k), m)
            got = dev.gcode_merge(c_off, c_pts, None, 1, True)
            want = MD.merge_numpy(c_off, c_pts, None, 1, True)
            res["equals_sequential_definition"] = {"paths": len(c_off) - 1, "equal": bool(all(np.array_equal(x, y) for x, y in zip(got[:5], want[:5])) and got[5] == want[5])}
    finally:
        dev.close()
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
