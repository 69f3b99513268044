"""What --simplify-mm costs and saves (csrc/gcode_simplify.hip), on the input it is for: --curves flattened circles and Lissajous curves of 64 .. 512 points
each on an A4 sheet, plus one stroke of --long points (a smooth curve with one step of noise), at tolerances of 0, 1 and 4 steps.  Per tolerance: the
orip_gcode_simplify call on the uploaded step polylines by the host clock (the call ends in a stream synchronisation; the upload of the input is inside it),
medians of --reps after one warm-up call; its level and emit kernels' times (orip_prof_get, in a run of their own); rounds; points in and out; and the pieces and bytes of the whole stream (orip.gcode.build_stream_from_gcode on the same strokes) against the stream without the
option.  At --check-size the call is compared with the sequential definition (tests/simplify_double.py).
usage: python tools/time_simplify.py [--curves N] [--long N] [--reps K] [--check-size N] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

STEPS_PER_MM = 40.0


def drawing(curves, long_points, seed=5):
    """(off, pts_mm): `curves` closed curves of 64 .. 512 points, radius 2 .. 12 mm, every other one a 3:2 Lissajous figure, then (long_points > 0) one
    93:87 Lissajous curve across the sheet through long_points points (two steps apart at 10^6), each moved by up to one step"""
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(curves):
        m = int(rng.integers(64, 513))
        t = np.linspace(0.0, 2.0 * np.pi, m)
        r = rng.uniform(2.0, 12.0); cx = rng.uniform(15.0, 195.0); cy = rng.uniform(15.0, 282.0)
        parts.append(np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1) if k % 2 == 0 else np.stack([cx + r * np.sin(3.0 * t), cy + r * np.sin(2.0 * t + 0.5)], 1))
    if long_points:
        t = np.linspace(0.0, 2.0 * np.pi, long_points)
        P = np.stack([105.0 + 90.0 * np.sin(93.0 * t + 0.5), 148.5 + 130.0 * np.sin(87.0 * t)], 1)
        parts.append(P + rng.integers(-1, 2, P.shape) / STEPS_PER_MM)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return off, np.concatenate(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", type=int, default=10000)
    ap.add_argument("--long", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-size", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip.device import Device
    from orip import gcode as GC
    import simplify_double as SD
    off_mm, pts_mm = drawing(a.curves, a.long)
    W, H = GC.target_size(GC.GcodeOptions())
    m = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=STEPS_PER_MM, W=W, H=H, invert_y=0)
    res = {"curves": a.curves, "long_points": a.long, "reps": a.reps, "tolerances": {}}
    dev = Device(0)
    try:
        off, pts = dev.gcode_to_steps(off_mm, pts_mm, m)                    # the step polylines: what the pass sees (points equal to the one before are gone)
        res["strokes"], res["points"] = len(off) - 1, len(pts)
        plain, pinfo = GC.build_stream_from_gcode((off_mm, pts_mm), GC.GcodeOptions(), dev)
        res["without"] = {"pieces": pinfo["pieces"], "bytes": pinfo["bytes"], "moves": pinfo["moves"]}
        for steps in (0, 1, 4):
            tol4 = 4 * steps
            call, kern = [], {"k_sp_level": [], "k_sp_emit": []}
            for rep in range(a.reps + 1):
                t0 = time.perf_counter(); out = dev.gcode_simplify(off, pts, tol4); t1 = time.perf_counter()
                if rep:
                    call.append(t1 - t0)
            raw = []
            st = np.zeros(4, np.int64)
            o = np.ascontiguousarray(off, np.int64); p = np.ascontiguousarray(pts, np.int32)
            for rep in range(a.reps + 1):                                     # the entry point alone: upload, kernels, the batched reads; no fetch
                t0 = time.perf_counter()
                dev._ck(dev.L.orip_gcode_simplify(dev.h, o.ctypes.data, p.ctypes.data, len(o) - 1, tol4, st.ctypes.data))
                t1 = time.perf_counter()
                if rep:
                    raw.append(t1 - t0)
            for rep in range(a.reps):                                         # the kernels, in runs of their own: every timed scope ends in an event wait
                dev.prof_reset(); dev.prof_enable(True)
                dev.gcode_simplify(off, pts, tol4)
                dev.prof_enable(False)
                for k in kern:
                    kern[k].append(dev.prof_get(k)[0] * 1e-3)
            data, info = GC.build_stream_from_gcode((off_mm, pts_mm), GC.GcodeOptions(simplify_mm=steps / STEPS_PER_MM), dev)
            res["tolerances"][str(steps)] = {
                "tol4": tol4, "entry_point_s_median": float(np.median(raw)), "entry_point_s_min_max": [float(min(raw)), float(max(raw))],
                "call_with_fetch_s_median": float(np.median(call)), "kernels_s_median": {k: float(np.median(v)) for k, v in kern.items()},
                "rounds": out[3]["rounds"], "points_in": out[3]["points_in"], "points_out": out[3]["points_out"], "simplify": info["simplify"],
                "pieces": info["pieces"], "bytes": info["bytes"], "moves": info["moves"]}
        if a.check_size:
            c_off, c_pts = dev.gcode_to_steps(*drawing(max(a.check_size // 300, 1), a.check_size), m)
            got = dev.gcode_simplify(c_off, c_pts, 4)
            want = SD.simplify_numpy(c_off, c_pts, 4)
            res["equals_sequential_definition"] = {"points": len(c_pts), "rounds": got[3]["rounds"],
                                                   "equal": bool(all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3])) and got[3]["points_out"] == want[3]["points_out"])}
    finally:
        dev.close()
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
