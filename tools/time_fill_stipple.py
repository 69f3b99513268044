"""What the fill stipple costs (csrc/fill_stipple.hip), beside the hatch on the same layers: the workload of tools/time_fill.py -- a synthetic 1414 x 2000
image (--height, --width) of four layers goes through stages 02 - 12 on the A4 canvas at 40 pixels per mm (8400 x 11880, 10 mm margins), which leaves the
four masks resident.  Then orip_fill_stipple runs on the resident mask of every layer at pitch 1 mm and 0.5 mm (stagger lattice, serpentine), with the
image's grey as tone and flat (tone NULL), with the radii fill_layers would pass (inset 0.3 mm, tone radius half the pitch, in source pixels), and the
dots are fetched: the call (the tone's upload and its read-backs inside) and the fetch by the host clock, summed over the four layers, median of --reps after
one warm-up; the phases (orip_prof_get, in runs of their own); the five counts per layer.  Beside it orip_fill_mask (the hatch at 45 degrees, spacing = the
pitch, inset 12, min_len 20, serpentine, along) on the same four layers, the same way.
usage: python tools/time_fill_stipple.py [--height H] [--width W] [--reps K] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT)
import numpy as np

PHASES = ("fs_verdict", "fs_emit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2000)
    ap.add_argument("--width", type=int, default=1414)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from orip import lib, stages as S
    from orip.config import Config, canvas_size_px
    from orip.device import Device, _p
    from orip.svg import hatch_direction_vector, stipple_lattice
    from orip.synth import layer_names, synth_image
    K = 4
    cfg = Config(); cfg.color_names = layer_names(K)
    W, H = canvas_size_px(cfg)
    place = S.fill_placement(cfg, a.width, a.height)
    num, den = place[:2]
    img = synth_image(a.height, a.width, K, seed=3, sigma=5.0)
    grey = np.ascontiguousarray((img.astype(np.uint16).sum(2) // 3).astype(np.uint8))
    res = {"source": [a.width, a.height], "canvas": [W, H], "placement": list(place), "reps": a.reps, "runs": {}}
    dev = Device(0)
    try:
        S.run_path(img, cfg, dev, fetch_ops=False)
        u = hatch_direction_vector(45)
        for pitch in (40, 20):
            lattice = stipple_lattice(pitch, "stagger")
            clear_rad, tone_rad = -((-12 * den) // num), min((pitch // 2 * den) // num, lib.FILL_STIPPLE_RAD_MAX)

            def hatch(l):
                st = np.zeros(len(lib.FILL_STATS), np.int64)
                t0 = time.perf_counter()
                dev._ck(dev.L.orip_fill_mask(dev.h, None, l, a.height, a.width, W, H, *place, *u, pitch, 12, 20, lib.FILL_SERPENTINE | lib.FILL_ALONG, _p(st)))
                t1 = time.perf_counter()
                seg = np.zeros((max(int(st[5]), 1), 4), np.int32)
                dev._ck(dev.L.orip_fill_fetch(dev.h, _p(seg)))
                return t1 - t0, time.perf_counter() - t1, dict(zip(lib.FILL_STATS, (int(v) for v in st)))

            def stipple(l, tone):
                st = np.zeros(len(lib.FILL_STIPPLE_STATS), np.int64)
                t0 = time.perf_counter()
                dev._ck(dev.L.orip_fill_stipple(dev.h, None, l, _p(grey) if tone else None, a.height, a.width, W, H, *place, *lattice, clear_rad, tone_rad, 0, 255,
                                                lib.FILL_STIPPLE_SERPENTINE, _p(st)))
                t1 = time.perf_counter()
                xy = np.zeros((max(int(st[4]), 1), 2), np.int32)
                dev._ck(dev.L.orip_fill_stipple_fetch(dev.h, _p(xy)))
                return t1 - t0, time.perf_counter() - t1, dict(zip(lib.FILL_STIPPLE_STATS, (int(v) for v in st)))

            def timed(fn):
                t_call, t_fetch = [], []
                for rep in range(a.reps + 1):
                    out = [fn(l) for l in range(K)]
                    if rep:
                        t_call.append(sum(o[0] for o in out)); t_fetch.append(sum(o[1] for o in out))
                return {"stats": [o[2] for o in out], "call_s_median": float(np.median(t_call)), "call_s_min_max": [float(min(t_call)), float(max(t_call))],
                        "fetch_s_median": float(np.median(t_fetch))}
            h = timed(hatch)
            print(f"pitch {pitch}: hatch at 45 degrees, four layers: call {h['call_s_median'] * 1e3:.2f} ms, fetch {h['fetch_s_median'] * 1e3:.2f} ms, "
                  f"{sum(s['segments'] for s in h['stats'])} segments")
            res["runs"][f"hatch_{pitch}"] = h
            for tone in (True, False):
                r = timed(lambda l: stipple(l, tone))
                kern = {k: [] for k in PHASES}
                for rep in range(a.reps):
                    dev.prof_reset(); dev.prof_enable(True)
                    for l in range(K):
                        stipple(l, tone)
                    dev.prof_enable(False)
                    for k in kern:
                        kern[k].append(dev.prof_get(k)[0] * 1e-3)
                r.update(lattice=list(lattice), clear_rad=clear_rad, tone_rad=tone_rad, tone=tone, phases_s_median={k: float(np.median(v)) for k, v in kern.items()})
                print(f"pitch {pitch}, {'tone' if tone else 'flat'} (lattice {lattice}, clear {clear_rad}, tone radius {tone_rad}), four layers: call {r['call_s_median'] * 1e3:.2f} ms, "
                      f"fetch {r['fetch_s_median'] * 1e3:.2f} ms, {sum(s['dots'] for s in r['stats'])} dots of {sum(s['ink'] for s in r['stats'])} ink of "
                      f"{sum(s['candidates'] for s in r['stats'])} candidates; phases " + ", ".join(f"{k} {v * 1e3:.2f}" for k, v in r["phases_s_median"].items()) + " ms")
                res["runs"][f"stipple_{pitch}_{'tone' if tone else 'flat'}"] = r
    finally:
        dev.close()
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
