"""The time of the hatch at an angle (csrc/hatch_angle.hip) beside the hatch it stands next to (csrc/hatch.hip, the yardstick: existing code), on the same
seeded drawing at the same spacing and inset: --groups filled star polygons of 10 edges (default 5000), radius 0.5 .. 3 mm, spread over an A4 page at 40
steps per mm, 0.5 mm spacing, the default inset, serpentine, one family of lines.
Per call: flatten and fit (not timed), then the hatch, after a warm-up run, --reps timed runs, median and spread; the kernels' own times from the profiling
scopes; the ratio of the medians.  The result of the new call is checked against the sequential double (tests/hatch_angle_double.py) by equality.
usage: python tools/time_hatch_angle.py [--groups N] [--reps R] [--angles A,B,..] [--lib FILE] [--out FILE.json]
--lib FILE loads another build of the library, so that two builds can be timed from one tree."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import numpy as np

import hatch_double as HD
import hatch_angle_double as HA

SPM, SPACING, INSET = 40.0, 20, 27
FLAGS = HD.HORIZONTAL | HD.SERPENTINE
KERNELS_PLAIN = ("k_ht_quant", "k_ht_cross_count", "k_ht_cross_fill", "k_ht_sort_wave", "k_ht_sort_block", "ht_sort_segmented", "k_ht_pairs", "k_ht_emit")
KERNELS_ANGLE = ("k_ha_quant", "k_ha_cross_count", "k_ha_cross_fill", "k_ha_sort_wave", "k_ha_sort_block", "ha_sort_merge", "k_ha_pairs", "k_ha_emit")


def many_polygons(n_groups, seed=1):
    rng = np.random.default_rng(seed)
    return [[HD.star(rng, rng.integers(130, 8270), rng.integers(130, 11750), rng.integers(20, 121), 10)] for _ in range(n_groups)]


def measure(dev, table, call, kernels, reps):
    runs = []
    for r in range(reps + 1):                                    # the first run is the warm-up: code objects, every buffer at its size
        dev.svg_flatten(table, 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
        t0 = time.perf_counter(); st = call(); dt = time.perf_counter() - t0
        if r:
            runs.append(dt)
    dev.svg_flatten(table, 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    dev.prof_reset(); dev.prof_enable(True); call(); dev.prof_enable(False)
    return {"counts": st, "hatch_s": {"median": float(np.median(runs)), "min": float(min(runs)), "max": float(max(runs))}, "kernel_ms": {k: dev.prof_get(k)[0] for k in kernels}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--angles", default="0,30,45")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip import lib
    if a.lib:
        lib.LIB_PATH = os.path.abspath(a.lib)
    from orip.device import Device
    from orip.svg import hatch_direction_vector
    groups = many_polygons(a.groups)
    table = HD.polys_table([[p / SPM for p in g] for g in groups])
    n_pts = int(table.sub_off[-1]) + table.n_sub
    dev = Device(0)
    res = {"steps_per_mm": SPM, "spacing_steps": SPACING, "inset_steps": INSET, "reps": a.reps, "lib": a.lib, "groups": a.groups, "edges": n_pts, "angle": {}}
    try:
        res["plain"] = measure(dev, table, lambda: dev.svg_hatch(table.fill_group, SPM, SPACING, INSET, FLAGS), KERNELS_PLAIN, a.reps)
        for ang in (float(v) for v in a.angles.split(",")):
            u = hatch_direction_vector(ang)
            r = measure(dev, table, lambda: dev.svg_hatch_angle(table.fill_group, SPM, SPACING, INSET, u, FLAGS), KERNELS_ANGLE, a.reps)
            off, pts = dev.svg_paths()
            t0 = time.perf_counter()
            want, wst = HA.hatch_segments_angle(off[:table.n_sub + 1], HA.quantise(pts[:n_pts], SPM), table.fill_group, SPACING, INSET, u, FLAGS)
            r["double_s"] = time.perf_counter() - t0
            assert r["counts"] == wst and np.array_equal(np.rint(pts[n_pts:] * SPM).astype(np.int64).reshape(-1, 4), want), "the device and the double disagree"
            r["u"] = list(u); r["ratio_to_plain"] = r["hatch_s"]["median"] / res["plain"]["hatch_s"]["median"]
            res["angle"][f"{ang:g}"] = r
    finally:
        dev.close()
    show = lambda name, r: print(f"{name}: {json.dumps(r['counts'])}\n  hatch median {1e3 * r['hatch_s']['median']:.3f} ms  min {1e3 * r['hatch_s']['min']:.3f}  max {1e3 * r['hatch_s']['max']:.3f}"
                                 f"\n  kernel ms: {json.dumps(r['kernel_ms'])}")
    print(f"{a.groups} groups, {n_pts} edges; {a.reps} runs after warm-up")
    show("orip_svg_hatch (horizontal)", res["plain"])
    for k, r in res["angle"].items():
        show(f"orip_svg_hatch_angle {k} deg u={tuple(r['u'])}", r)
        print(f"  ratio to orip_svg_hatch {r['ratio_to_plain']:.2f}; the sequential double {r['double_s']:.1f} s")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
