"""Where the time of svg2stream goes (orip/svg.py, csrc/svg.hip), on a seeded SVG of --segments cubic segments (short strokes of 1-4 cubics spread over a
page, in file order unrelated to position): parse, flatten, bbox, fit, to_steps, order, plan, codes, pack through build_stream_from_svg, after a warm-up
run, --reps timed runs, median and spread (min .. max) per step; next to it the host-only cost of parsing and the kernels' own times.
usage: python tools/time_svg.py [--segments N] [--reps R] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT)
import numpy as np

STEPS = ("parse_svg", "flatten", "bbox", "fit", "fetch_paths", "to_steps", "order", "plan", "codes", "pack")


def synth_svg(n_seg, seed=1, w=2000.0, h=2800.0):
    rng = np.random.default_rng(seed)
    out = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{w:g}" height="{h:g}">']
    left = n_seg
    while left > 0:
        k = min(left, int(rng.integers(1, 5)))
        p = rng.uniform([20, 20], [w - 20, h - 20])
        d = [f"M{p[0]:.2f} {p[1]:.2f}"]
        for _ in range(k):
            q = rng.normal(0, 12.0, (3, 2))
            d.append("c" + " ".join(f"{v:.2f}" for v in np.cumsum(q, 0).reshape(-1)))
        out.append(f'<path d="{"".join(d)}"/>')
        left -= k
    out.append("</svg>")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip.device import Device
    from orip import svg as SV
    text = synth_svg(a.segments)
    opts = SV.SvgOptions()
    dev = Device(0)
    try:
        SV.build_stream_from_svg(synth_svg(2000, seed=2), opts, dev)         # code objects, first buffers
        data0, info = SV.build_stream_from_svg(text, opts, dev)              # warm-up at size: every buffer has grown
        runs, whole = [], []
        for _ in range(a.reps):
            tm = {}
            t0 = time.perf_counter(); data, info = SV.build_stream_from_svg(text, opts, dev, timings=tm); whole.append(time.perf_counter() - t0)
            assert data == data0
            runs.append(tm)
        dev.prof_reset(); dev.prof_enable(True); SV.build_stream_from_svg(text, opts, dev); dev.prof_enable(False)
        kern = {k: dev.prof_get(k)[0] for k in ("k_svg_count", "k_svg_emit", "k_svg_fit", "k_gc_points", "k_gc_emit", "k_gc_chain", "k_seg_codes", "k_pk_bytes")}
    finally:
        dev.close()
    table = SV.parse_svg(text)
    res = {"segments": a.segments, "svg_bytes": len(text), "reps": a.reps, "subpaths": table.n_sub, "points": int(info["pen_down_moves"]) + table.n_sub, "paths": info["paths"],
           "steps": info["steps"], "stream_bytes": len(data0), "tol_raw": info["tol_raw"], "flattens": info["flattens"], "kernel_ms": kern,
           "whole_s": {"median": float(np.median(whole)), "min": float(min(whole)), "max": float(max(whole))}, "stages_s": {}}
    for k in STEPS:
        v = [r.get(k, 0.0) for r in runs]
        res["stages_s"][k] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    print(f"{a.segments} cubic segments, {table.n_sub} subpaths -> {res['points']} points, {info['paths']} step paths, {info['steps']} steps, {len(data0)} bytes; {a.reps} runs after warm-up")
    print(f"{'step':12s} {'median ms':>10s} {'min':>9s} {'max':>9s}")
    for k in STEPS:
        s = res["stages_s"][k]
        print(f"{k:12s} {1e3 * s['median']:10.2f} {1e3 * s['min']:9.2f} {1e3 * s['max']:9.2f}")
    s = res["whole_s"]
    print(f"{'whole':12s} {1e3 * s['median']:10.2f} {1e3 * s['min']:9.2f} {1e3 * s['max']:9.2f}")
    print("kernel ms:", json.dumps(kern))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
