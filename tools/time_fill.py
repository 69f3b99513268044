"""What fill_layers costs (csrc/fill.hip), beside stage 12 on the same layers: a synthetic 1414 x 2000 image (--height, --width) of four layers goes through
stages 02 - 12 on the A4 canvas at 40 pixels per mm (8400 x 11880, 10 mm margins), which leaves the four masks and the four layers' lines resident.  Then,
per angle 0, 45 and 90 degrees, orip_fill_mask runs on the resident mask of every layer (spacing 1 mm = 40 pixels, inset 12, min_len 20, serpentine,
along) and the segments are fetched: the call (its three read-backs inside) and the fetch by the host clock, summed over the four layers, median of
--reps after one warm-up; the phases (orip_prof_get, in runs of their own); the six counts per layer.  Beside it orip_plot_order (stage 12) of the same
four layers, one after the other, the same way.  --cross adds the across family.
usage: python tools/time_fill.py [--height H] [--width W] [--reps K] [--spacing PX] [--cross] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT)
import numpy as np

PHASES = ("fl_sample", "fl_count", "fl_runs", "fl_emit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2000)
    ap.add_argument("--width", type=int, default=1414)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spacing", type=int, default=40)
    ap.add_argument("--cross", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_times.json"))
    a = ap.parse_args()
    from orip import lib, stages as S
    from orip.config import Config, canvas_size_px
    from orip.device import Device, _p
    from orip.svg import hatch_direction_vector
    from orip.synth import layer_names, synth_image
    K = 4
    cfg = Config(); cfg.color_names = layer_names(K)
    W, H = canvas_size_px(cfg)
    place = S.fill_placement(cfg, a.width, a.height)
    flags = lib.FILL_SERPENTINE | lib.FILL_ALONG | (lib.FILL_ACROSS if a.cross else 0)
    res = {"source": [a.width, a.height], "canvas": [W, H], "placement": list(place), "spacing": a.spacing, "inset": 12, "min_len": 20, "flags": flags, "reps": a.reps, "angles": {}}
    dev = Device(0)
    try:
        S.run_path(synth_image(a.height, a.width, K, seed=3, sigma=5.0), cfg, dev, fetch_ops=False)
        R12 = S.r_insert12(cfg)
        t12 = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            n_ops = [len(dev.plot_order(l, R12)) for l in range(K)]
            if rep:
                t12.append(time.perf_counter() - t0)
        res["stage12"] = {"ops": n_ops, "s_median": float(np.median(t12)), "s_min_max": [float(min(t12)), float(max(t12))]}
        print(f"stage 12, four layers: {res['stage12']['s_median'] * 1e3:.2f} ms ({sum(n_ops)} ops)")
        for angle in (0, 45, 90):
            u = hatch_direction_vector(angle)

            def fill(l):
                st = np.zeros(len(lib.FILL_STATS), np.int64)
                t0 = time.perf_counter()
                dev._ck(dev.L.orip_fill_mask(dev.h, None, l, a.height, a.width, W, H, *place, *u, a.spacing, 12, 20, flags, _p(st)))
                t1 = time.perf_counter()
                seg = np.zeros((max(int(st[5]), 1), 4), np.int32)
                dev._ck(dev.L.orip_fill_fetch(dev.h, _p(seg)))
                return t1 - t0, time.perf_counter() - t1, dict(zip(lib.FILL_STATS, (int(v) for v in st)))
            t_call, t_fetch = [], []
            for rep in range(a.reps + 1):
                out = [fill(l) for l in range(K)]
                if rep:
                    t_call.append(sum(o[0] for o in out)); t_fetch.append(sum(o[1] for o in out))
            kern = {k: [] for k in PHASES}
            for rep in range(a.reps):
                dev.prof_reset(); dev.prof_enable(True)
                for l in range(K):
                    fill(l)
                dev.prof_enable(False)
                for k in kern:
                    kern[k].append(dev.prof_get(k)[0] * 1e-3)
            r = {"u": list(u), "stats": [o[2] for o in out], "call_s_median": float(np.median(t_call)), "call_s_min_max": [float(min(t_call)), float(max(t_call))],
                 "fetch_s_median": float(np.median(t_fetch)), "phases_s_median": {k: float(np.median(v)) for k, v in kern.items()}}
            print(f"{angle} degrees, four layers: call {r['call_s_median'] * 1e3:.2f} ms, fetch {r['fetch_s_median'] * 1e3:.2f} ms, "
                  f"{sum(s['segments'] for s in r['stats'])} segments of {sum(s['runs'] for s in r['stats'])} runs on {sum(s['lines'] for s in r['stats'])} lines; phases "
                  + ", ".join(f"{k} {v * 1e3:.2f}" for k, v in r["phases_s_median"].items()) + " ms")
            res["angles"][str(angle)] = r
    finally:
        dev.close()
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
