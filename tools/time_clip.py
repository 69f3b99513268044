"""What --clip costs (csrc/gcode_clip.hip) next to the conversion it replaces, on the input it is for: a drawing of --points points in --paths paths on an
A4 sheet, too wide for it -- about a third of the points lie off the sheet.  orip_gcode_to_steps and orip_gcode_to_steps_clip run on the same paths in mm;
per call the host clock around it (each call ends in a stream synchronisation and a fetch of the result), medians of --reps after one warm-up run, and the
two timed kernels of each (orip_prof_get).  Then the whole tool (orip.gcode.build_stream_from_gcode) without and with the option, per step the host clock
of its lap.  At --check-size the clip is compared with the sequential definition (tests/clip_double.py).
usage: python tools/time_clip.py [--points N] [--paths N] [--reps K] [--check-size N] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def wide_drawing(points, paths, seed=7):
    """(off, pts_mm): `paths` random walks of points / paths points each, 1 mm a point at most, started anywhere in a band of 315 x 297 mm that reaches a
    quarter of a sheet's width over each side edge of A4: a third of it is off the sheet"""
    rng = np.random.default_rng(seed)
    k = max(2, points // paths)
    start = np.stack([rng.uniform(-52.5, 262.5, paths), rng.uniform(0.0, 297.0, paths)], 1)
    steps = rng.uniform(-1.0, 1.0, (paths, k, 2)); steps[:, 0] = 0.0
    pts = (start[:, None, :] + np.cumsum(steps, 1)).reshape(-1, 2)
    return np.arange(paths + 1, dtype=np.int64) * k, np.ascontiguousarray(pts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--paths", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-size", type=int, default=20000)
    ap.add_argument("--tool-points", type=int, default=100000, help="the size of the whole-tool runs (the order is a chain of dependent searches)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip.device import Device
    from orip import gcode as GC
    import clip_double as CD
    off, pts = wide_drawing(a.points, a.paths)
    W, H = GC.target_size(GC.GcodeOptions())
    m = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=40.0, W=W, H=H, invert_y=0)
    rect = (0, 0, W - 1, H - 1)
    off_sheet = float(((pts[:, 0] < 0) | (pts[:, 0] > 210.0) | (pts[:, 1] < 0) | (pts[:, 1] > 297.0)).mean())
    res = {"points": int(off[-1]), "paths": a.paths, "share_of_points_off_the_sheet": off_sheet}
    dev = Device(0)
    try:
        calls = {"to_steps": (lambda: dev.gcode_to_steps(off, pts, m), ("k_gc_points", "k_gc_emit")),
                 "to_steps_clip": (lambda: dev.gcode_to_steps_clip(off, pts, m, rect), ("k_cl_segments", "k_cl_emit"))}
        for name, (fn, kernels) in calls.items():
            plain, kern = [], {k: [] for k in kernels}
            for rep in range(a.reps + 1):                                      # the first run loads code objects and grows buffers
                t0 = time.perf_counter(); out = fn(); t1 = time.perf_counter()
                if rep:
                    plain.append(t1 - t0)
            for rep in range(a.reps + 1):                                      # the kernels in runs of their own: with the profile on, every timed kernel is followed by an event wait
                dev.prof_reset(); dev.prof_enable(rep > 0)
                fn()
                dev.prof_enable(False)
                if rep:
                    for k in kernels:
                        kern[k].append(dev.prof_get(k)[0] * 1e-3)
            res[name] = {"call_with_fetch_s_median": float(np.median(plain)), "call_with_fetch_s_min": float(np.min(plain)), "kernels_s_median": {k: float(np.median(v)) for k, v in kern.items()},
                         "paths_out": len(out[0]) - 1, "points_out": len(out[1]), "reps": a.reps}
            if name == "to_steps_clip":
                res[name]["stats"] = out[2]
        # the whole tool without and with the option
        t_off, t_pts = wide_drawing(a.tool_points, max(1, a.tool_points // 10))
        for name, clip in (("tool_without", False), ("tool_with", True)):
            laps, whole = [], []
            for rep in range(min(a.reps, 3) + 1):
                tm = {}
                t0 = time.perf_counter(); data, info = GC.build_stream_from_gcode((t_off, t_pts), GC.GcodeOptions(clip=clip), dev, timings=tm); t1 = time.perf_counter()
                if rep:
                    laps.append(tm); whole.append(t1 - t0)
            res[name] = {"points": int(t_off[-1]), "whole_s_median": float(np.median(whole)), "laps_s_median": {k: float(np.median([l[k] for l in laps])) for k in laps[0]},
                         "paths": info["paths"], "steps": info["steps"], "bytes": len(data)}
            if clip:
                res[name]["clip"] = {k: v for k, v in info["clip"].items() if k != "rect"}
        if a.check_size:
            c_off, c_pts = wide_drawing(a.check_size, max(1, a.check_size // 10))
            g_off, g_pts, g_st = dev.gcode_to_steps_clip(c_off, c_pts, m, rect)
            g_src = dev.gcode_steps_source(len(g_off) - 1)
            want = CD.clip_numpy(c_off, c_pts, m, rect)
            res["equals_sequential_definition"] = {"points": int(c_off[-1]), "stats": want[3],
                                                   "equal": bool(all(np.array_equal(x, y) for x, y in zip((g_off, g_pts, g_src), want[:3])) and g_st == want[3])}
    finally:
        dev.close()
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
