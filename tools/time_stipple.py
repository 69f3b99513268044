"""What --stipple-mm costs (csrc/gcode_stipple.hip), beside orip_svg_hatch on the same drawing, on three inputs: "polygons", --polygons 64-gons of radius
1000 steps side by side, each a shape of its own; "single", hatch_double.single_polygon(): one polygon of --edges edges over an A4 page; "squares",
--squares x --squares squares 300 wide and 150 apart, each painted over its neighbours, with ORIP_STIPPLE_OCCLUDE.  Each is flattened and fitted on the
device; then orip_svg_stipple runs on the fitted paths as rings (lattice (40, 35, 20): --stipple-mm 1 at 40 steps per mm, stagger; inset 27; serpentine),
then orip_svg_hatch (spacing 40, inset 27, horizontal, serpentine).  Per input: both calls by the host clock (each ends in a stream synchronisation; the
stipple's read-backs and the fetch of the dots are inside it), median of --reps after one warm-up (every repetition flattens anew: the hatch appends to
the resident paths); the stipple's phases (orip_prof_get, in runs of their own); the seven counts; and, up to --check-points lattice-point-edge tests,
the comparison with the sequential definition (tests/stipple_double.py).
usage: python tools/time_stipple.py [--polygons N] [--edges N] [--squares N] [--reps K] [--lib FILE] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

LATTICE, INSET, SPACING = (40, 35, 20), 27, 40
PHASES = ("st_test", "st_emit")


def polygons(n):
    import hatch_link_cases as LC
    side = int(np.ceil(np.sqrt(n)))
    return [[np.asarray(LC.ngon(1100 + 2200 * (k % side), 1100 + 2200 * (k // side), 1000, 64), np.float64)] for k in range(n)]


def squares(side):
    return [[np.asarray([(100 + 150 * i, 100 + 150 * j), (400 + 150 * i, 100 + 150 * j), (400 + 150 * i, 400 + 150 * j), (100 + 150 * i, 400 + 150 * j)], np.float64)]
            for j in range(side) for i in range(side)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--polygons", type=int, default=1000)
    ap.add_argument("--edges", type=int, default=100000)
    ap.add_argument("--squares", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-points", type=int, default=20000000)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stipple_times.json"))
    a = ap.parse_args()
    from orip import lib
    if a.lib:
        lib.LIB_PATH = os.path.abspath(a.lib)
    from orip.device import Device
    import hatch_double as HD
    import occlude_double as OD
    import stipple_double as SD
    side = int(np.ceil(np.sqrt(a.polygons)))
    inputs = {"polygons": (polygons(a.polygons), 2200 * side + 200, SD.SERPENTINE), "single": ([[HD.single_polygon(a.edges).astype(np.float64)]], 12000, SD.SERPENTINE),
              "squares": (squares(a.squares), 150 * a.squares + 500, SD.SERPENTINE | SD.OCCLUDE)}
    res = {"polygons": a.polygons, "edges": a.edges, "squares": a.squares, "reps": a.reps, "lattice": LATTICE, "inset": INSET, "hatch_spacing": SPACING, "lib": a.lib, "inputs": {}}
    dev = Device(0)
    try:
        for name, (polys, size, flags) in inputs.items():
            table = HD.polys_table(polys)
            fg = np.arange(table.n_sub, dtype=np.int32)
            m = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=1.0, W=size, H=size, invert_y=0)
            rect = (0, 0, size - 1, size - 1)

            def prepare():
                dev.svg_flatten(table, 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)

            def stipple():
                t0 = time.perf_counter()
                out = dev.svg_stipple(fg, fg, m, True, LATTICE, INSET, rect, flags)
                return time.perf_counter() - t0, out

            def hatch():
                t0 = time.perf_counter()
                st = dev.svg_hatch(fg, 1.0, SPACING, INSET, HD.HORIZONTAL | HD.SERPENTINE)
                return time.perf_counter() - t0, st
            t_st, t_ht = [], []
            for rep in range(a.reps + 1):
                prepare()
                ts, out = stipple()
                th, hst = hatch()
                if rep:
                    t_st.append(ts); t_ht.append(th)
            r = {"subpaths": int(table.n_sub), "ring_points": int(table.sub_off[-1] + table.n_sub), "stats": out[2], "hatch": {k: int(v) for k, v in hst.items()},
                 "stipple_s_median": float(np.median(t_st)), "stipple_s_min_max": [float(min(t_st)), float(max(t_st))], "hatch_s_median": float(np.median(t_ht))}
            kern = {k: [] for k in PHASES}
            for rep in range(a.reps):
                prepare()
                dev.prof_reset(); dev.prof_enable(True); stipple(); dev.prof_enable(False)
                for k in kern:
                    kern[k].append(dev.prof_get(k)[0] * 1e-3)
            r["phases_s_median"] = {k: float(np.median(v)) for k, v in kern.items()}
            work = 2 * out[2]["candidates"] * (r["ring_points"] // table.n_sub) * (table.n_sub if flags & SD.OCCLUDE else 1)
            if work <= a.check_points:                                          # the double tests every lattice point of a box against every edge of its shape, and of every shape above
                prepare()
                p_off, p_mm = dev.svg_paths(table.n_sub)
                r_off, r_pts = OD.rings_to_steps(p_off, p_mm, fg.tolist(), m, True)
                want = SD.stipple(r_off, r_pts, fg, LATTICE, INSET, rect, flags)
                r["equals_sequential_definition"] = bool(np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1]) and out[2] == want[2])
            print(f"{name}: stipple call {r['stipple_s_median'] * 1e3:.2f} ms ({out[2]['dots']} dots of {out[2]['candidates']} candidates in {out[2]['groups']} shapes), "
                  f"hatch call {r['hatch_s_median'] * 1e3:.2f} ms ({r['hatch']['segments']} lines)")
            res["inputs"][name] = r
    finally:
        dev.close()
    print(json.dumps(res, indent=2))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
