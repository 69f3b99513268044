"""What --improve-order costs and saves (csrc/gcode_improve.hip), on two inputs: a seeded random plot of --strokes short strokes (300 steps at most) on an
A4 sheet, through orip.gcode.build_stream_from_gcode with and without --allow-reverse, and an SVG of filled discs hatched at --hatch-mm, through
orip.svg.build_stream_from_svg.  Each whole tool runs without and with the option; per step the host clock of its lap (each ends in a stream
synchronisation), medians of --reps after one warm-up run; the rounds, the time per round, the pen-up steps before and after, and the steps of both streams
as the stage-14 decoder counts them.  The floor of a round -- two launches, the reduction of the records and the position map, next to no evaluation -- is
the time per round of the call alone on 64 strokes; the evaluation's share at --strokes is what is left above it.
usage: python tools/time_improve.py [--strokes N] [--reps K] [--hatch-mm S] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def random_strokes(m, seed=7, steps_per_mm=40.0, longest=300):
    """(off, pts_mm): m two-point strokes inside the A4 margins, none longer than `longest` steps per axis"""
    rng = np.random.default_rng(seed)
    a = np.stack([rng.uniform(10, 200, m), rng.uniform(10, 287, m)], 1)
    b = a + rng.uniform(-longest, longest, (m, 2)) / steps_per_mm
    return np.arange(m + 1) * 2, np.stack([a, np.clip(b, 5, [205, 292])], 1).reshape(-1, 2)


def hatched_discs(seed=8, count=40):
    rng = np.random.default_rng(seed)
    body = "".join('<circle cx="%.1f" cy="%.1f" r="%.1f" fill="#000" stroke="#000"/>' % (rng.uniform(20, 190), rng.uniform(20, 270), rng.uniform(4, 14)) for _ in range(count))
    return ('<svg xmlns="http://www.w3.org/2000/svg" width="210mm" height="297mm" viewBox="0 0 210 297">%s</svg>' % body).encode()


def timed(build, reps):
    laps, whole = [], []
    for rep in range(reps + 1):
        tm = {}
        t0 = time.perf_counter(); data, info = build(tm); t1 = time.perf_counter()
        if rep:                                                               # the first run loads code objects and grows buffers
            laps.append(tm); whole.append(t1 - t0)
    return data, info, {"whole_s_median": float(np.median(whole)), "laps_s_median": {k: float(np.median([l[k] for l in laps])) for k in laps[0]}, "reps": reps}


def report(dev, data, info, res):
    from orip import stream_preview as SP
    W, H = info["target"]
    st = SP.preview(dev, data, W, H, 600, 848, invert_y=True)[1]
    res.update(paths=info["paths"], steps_total=st["steps_total"], pen_down_segments=st["pen_down_segments"], bytes=len(data))
    if "improve" in info:
        res["improve"] = info["improve"]
        r = info["improve"]["rounds"]
        res["us_per_round"] = 1e6 * res["laps_s_median"]["improve"] / r if r else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strokes", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--hatch-mm", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip.device import Device
    from orip import gcode as GC, svg as SV
    import improve_cases as IC
    m = a.strokes
    res = {"strokes": m, "candidates_per_round": {"pairs_i_g": m * (m + 1), "candidates": 4 * m * (m + 1), "note": "3 M and, with reversal, 1 R per pair; 6 distances per pair"}}
    dev = Device(0)
    try:
        paths = random_strokes(m)
        for reverse in (False, True):
            for improve in (False, True):
                o = GC.GcodeOptions(allow_reverse=reverse, improve_order=improve)
                data, info, r = timed(lambda tm: GC.build_stream_from_gcode(paths, o, dev, timings=tm), a.reps)
                res["random_%s_%s" % ("reverse" if reverse else "forward", "with" if improve else "without")] = report(dev, data, info, r)
        svg = hatched_discs()
        for improve in (False, True):
            args = ["in.svg", "--no-preview", "--hatch-spacing-mm", str(a.hatch_mm), "--allow-reverse"] + (["--improve-order"] if improve else [])
            o = SV.options_from_args(SV.build_stream_argparser().parse_args(args))
            data, info, r = timed(lambda tm: SV.build_stream_from_svg(svg, o, dev, timings=tm), a.reps)
            res["hatched_svg_%s" % ("with" if improve else "without")] = report(dev, data, info, r)
        # the floor of a round: the call alone on 64 shuffled strokes, 32 rounds
        case = IC.random_plot(64, 1, reverse=True)
        t = []
        for rep in range(a.reps + 2):
            t0 = time.perf_counter(); out = dev.gcode_improve(*case[:5], True, case[5], 32); t1 = time.perf_counter()
            if rep:
                t.append(t1 - t0)
        res["floor"] = {"strokes": 64, "rounds": out[2]["rounds"], "us_per_round": 1e6 * float(np.median(t)) / 32, "note": "includes the call's copies and its two syncs"}
    finally:
        dev.close()
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
