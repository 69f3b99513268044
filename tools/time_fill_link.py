"""What fill connect costs (csrc/fill_link.hip), beside the fill it works on: tools/time_fill.py's workload -- a synthetic 1414 x 2000 image (--height, --width)
of four layers through stages 02 - 12 on the A4 canvas at 40 pixels per mm, which leaves the four masks resident.  Then, per angle 0, 45 and 90 degrees and
per layer, orip_fill_mask on the resident mask (spacing 1 mm = 40 pixels, inset 12, min_len 20, serpentine, along) and orip_fill_link behind it (reach =
--reach-mult x spacing, default 2: the front door's default), each with its fetch: the calls by the host clock, summed over the four layers, median of --reps
after one warm-up; the link's phases (orip_prof_get, in runs of their own); the seven counts per layer; and the ops of the fill -- one pen lift each --
before (segments) and after (paths_out).  --cross adds the across family.
usage: python tools/time_fill_link.py [--height H] [--width W] [--reps K] [--spacing PX] [--reach-mult M] [--cross] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT)
import numpy as np

PHASES = ("fk_count", "fk_elig", "fk_chain", "fk_emit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2000)
    ap.add_argument("--width", type=int, default=1414)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spacing", type=int, default=40)
    ap.add_argument("--reach-mult", type=int, default=2)
    ap.add_argument("--cross", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_link_times.json"))
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
    reach = a.reach_mult * a.spacing
    res = {"source": [a.width, a.height], "canvas": [W, H], "placement": list(place), "spacing": a.spacing, "inset": 12, "min_len": 20, "flags": flags, "reach": reach, "reps": a.reps,
           "angles": {}}
    dev = Device(0)
    try:
        S.run_path(synth_image(a.height, a.width, K, seed=3, sigma=5.0), cfg, dev, fetch_ops=False)
        for angle in (0, 45, 90):
            u = hatch_direction_vector(angle)

            def one(l):
                st = np.zeros(len(lib.FILL_STATS), np.int64); lst = np.zeros(len(lib.FILL_LINK_STATS), np.int64)
                t0 = time.perf_counter()
                dev._ck(dev.L.orip_fill_mask(dev.h, None, l, a.height, a.width, W, H, *place, *u, a.spacing, 12, 20, flags, _p(st)))
                t1 = time.perf_counter()
                dev._ck(dev.L.orip_fill_link(dev.h, None, l, a.height, a.width, *place, reach, _p(lst)))
                t2 = time.perf_counter()
                off = np.zeros(int(lst[4]) + 1, np.int64); pts = np.zeros((max(int(lst[5]), 1), 2), np.int32)
                dev._ck(dev.L.orip_fill_link_fetch(dev.h, _p(off), _p(pts)))
                return t1 - t0, t2 - t1, time.perf_counter() - t2, dict(zip(lib.FILL_LINK_STATS, (int(v) for v in lst)))
            t_fill, t_link, t_fetch = [], [], []
            for rep in range(a.reps + 1):
                out = [one(l) for l in range(K)]
                if rep:
                    t_fill.append(sum(o[0] for o in out)); t_link.append(sum(o[1] for o in out)); t_fetch.append(sum(o[2] for o in out))
            kern = {k: [] for k in PHASES}
            for rep in range(a.reps):
                dev.prof_reset(); dev.prof_enable(True)
                for l in range(K):
                    one(l)
                dev.prof_enable(False)
                for k in kern:
                    kern[k].append(dev.prof_get(k)[0] * 1e-3)
            stats = [o[3] for o in out]
            r = {"u": list(u), "stats": stats, "fill_call_s_median": float(np.median(t_fill)), "link_call_s_median": float(np.median(t_link)),
                 "link_call_s_min_max": [float(min(t_link)), float(max(t_link))], "link_fetch_s_median": float(np.median(t_fetch)),
                 "phases_s_median": {k: float(np.median(v)) for k, v in kern.items()}, "ops_before": sum(s["segments"] for s in stats), "ops_after": sum(s["paths_out"] for s in stats),
                 "link_steps": sum(s["link_steps"] for s in stats)}
            print(f"{angle} degrees, four layers: fill {r['fill_call_s_median'] * 1e3:.2f} ms, link {r['link_call_s_median'] * 1e3:.2f} ms, link fetch {r['link_fetch_s_median'] * 1e3:.2f} ms; "
                  f"pen lifts {r['ops_before']} -> {r['ops_after']} ({sum(s['in_reach'] for s in stats)} pairs in reach, {sum(s['eligible'] for s in stats)} eligible, "
                  f"{sum(s['links'] for s in stats)} links, {r['link_steps']} link steps); phases " + ", ".join(f"{k} {v * 1e3:.2f}" for k, v in r["phases_s_median"].items()) + " ms")
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
