"""Where the time of the hatch fill goes (csrc/hatch.hip), on two seeded drawings on an A4 page at 40 steps per mm, 0.5 mm spacing, the default inset, serpentine:
  many    --groups filled star polygons of 10 edges (default 100000 groups, 10^6 edges), radius 0.5 .. 3 mm, spread over the page
  single  one polygon of 100000 edges filling the page (tests/hatch_double.py: single_polygon), the case the reference's own time is recorded for
Per drawing: flatten, fit and hatch on the device after a warm-up run, --reps timed runs, median and spread; the kernels' own times; the result checked against
the numpy double (tests/hatch_double.py) by equality.  Beside them, as context only: the wall time of that numpy double on the same input, and for `single`
the wall time of the reference's hatch_fill recorded in tests/golden/golden_hatch.npz where the fixture was made (another machine's CPU).
usage: python tools/time_hatch.py [--groups N] [--reps R] [--lib FILE] [--out FILE.json]
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

SPM, SPACING, INSET = 40.0, 20, 27
KERNELS = ("k_ht_quant", "k_ht_cross_count", "k_ht_cross_fill", "k_ht_sort_wave", "k_ht_sort_block", "ht_sort_segmented", "k_ht_pairs", "k_ht_emit")


def many_polygons(n_groups, seed=1):
    rng = np.random.default_rng(seed)
    return [[HD.star(rng, rng.integers(130, 8270), rng.integers(130, 11750), rng.integers(20, 121), 10)] for _ in range(n_groups)]


def measure(dev, groups, reps):
    table = HD.polys_table([[p / SPM for p in g] for g in groups])
    flags = HD.HORIZONTAL | HD.SERPENTINE
    runs = []
    for r in range(reps + 1):                                    # the first run is the warm-up: code objects, every buffer at its size
        tm = {}
        t0 = time.perf_counter(); dev.svg_flatten(table, 1.0); tm["flatten"] = time.perf_counter() - t0
        t0 = time.perf_counter(); dev.svg_fit(1.0, 1.0, 0.0, 0.0); tm["fit"] = time.perf_counter() - t0
        t0 = time.perf_counter(); st = dev.svg_hatch(table.fill_group, SPM, SPACING, INSET, flags); tm["hatch"] = time.perf_counter() - t0
        if r:
            runs.append(tm)
    off, pts = dev.svg_paths()
    n_pts = int(table.sub_off[-1]) + table.n_sub
    dev.svg_flatten(table, 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    dev.prof_reset(); dev.prof_enable(True); dev.svg_hatch(table.fill_group, SPM, SPACING, INSET, flags); dev.prof_enable(False)
    kern = {k: dev.prof_get(k)[0] for k in KERNELS}
    t0 = time.perf_counter()
    want, wst = HD.hatch_segments(off[:table.n_sub + 1], HD.quantise(pts[:n_pts], SPM), table.fill_group, SPACING, INSET, flags)
    t_numpy = time.perf_counter() - t0
    got = np.rint(pts[n_pts:] * SPM).astype(np.int64).reshape(-1, 4)
    assert st == wst and np.array_equal(got, want), "the device and the numpy double disagree"
    res = {"groups": len(groups), "edges": n_pts, "counts": st, "kernel_ms": kern, "numpy_double_s": t_numpy, "stages_s": {}}
    for k in ("flatten", "fit", "hatch"):
        v = [r[k] for r in runs]
        res["stages_s"][k] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip import lib
    if a.lib:
        lib.LIB_PATH = os.path.abspath(a.lib)
    from orip.device import Device
    from util import load
    G = load("golden_hatch.npz")
    dev = Device(0)
    try:
        measure(dev, many_polygons(500, seed=2), 1)
        res = {"steps_per_mm": SPM, "spacing_steps": SPACING, "inset_steps": INSET, "reps": a.reps, "lib": a.lib,
               "many": measure(dev, many_polygons(a.groups), a.reps), "single": measure(dev, [[HD.single_polygon(100000)]], a.reps)}
    finally:
        dev.close()
    n_edges, spacing, inset, serp = (int(v) for v in G["time_single_prm"])
    if (n_edges, spacing, inset, serp) == (100000, SPACING, INSET, 1) and float(G["time_single_ref_s"][0]) > 0:
        res["single"]["reference_hatch_fill_s"] = float(G["time_single_ref_s"][0])
        assert int(G["time_single_segments"][0]) == res["single"]["counts"]["segments"]
    for name in ("many", "single"):
        r = res[name]
        print(f"{name}: {r['groups']} groups, {r['edges']} edges -> {r['counts']['lines']} lines, {r['counts']['crossings']} crossings, {r['counts']['segments']} segments; {a.reps} runs after warm-up")
        for k, s in r["stages_s"].items():
            print(f"  {k:8s} median {1e3 * s['median']:9.2f} ms   min {1e3 * s['min']:9.2f}   max {1e3 * s['max']:9.2f}")
        print("  kernel ms:", json.dumps(r["kernel_ms"]))
        print(f"  numpy double {1e3 * r['numpy_double_s']:.1f} ms" + (f", reference hatch_fill {r['reference_hatch_fill_s']:.1f} s (recorded with the fixture)" if "reference_hatch_fill_s" in r else ""))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
