"""What --hatch-connect costs (csrc/gcode_link.hip), on two drawings: "polygons", --polygons 64-gons of radius 1000 steps side by side, each a fill group of
its own (about 50 hatch lines each); "single", hatch_double.single_polygon(): one polygon of --edges edges over an A4 page.  Both are flattened, fitted,
hatched (spacing 40, inset 27, horizontal, serpentine) and converted on the device; then orip_svg_hatch_link runs on the resident strokes with the fitted
paths as rings, reach 80.  Per drawing: the hatch call and the link call by the host clock (each ends in a stream synchronisation; the link's read-backs are
inside it, the fetches are not), median of --reps after one warm-up (every repetition converts anew: the pass consumes its input); the link's phases
(orip_prof_get, in runs of their own); `lines -> paths_out` and the other counts; the pen lifts of the whole stream, strokes in the finished drawing, with
and without the option; and, up to --check-lines lines and five million pair-edge tests, the comparison with the sequential definition (tests/hatch_link_double.py).
usage: python tools/time_hatch_link.py [--polygons N] [--edges N] [--reps K] [--lib FILE] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SPACING, INSET, REACH = 40, 27, 80
PHASES = ("hl_sort", "hl_count", "hl_elig", "hl_jump", "hl_emit")


def polygons(n):
    import hatch_link_cases as LC
    side = int(np.ceil(np.sqrt(n)))
    return [[np.asarray(LC.ngon(1100 + 2200 * (k % side), 1100 + 2200 * (k // side), 1000, 64), np.float64)] for k in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--polygons", type=int, default=1000)
    ap.add_argument("--edges", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-lines", type=int, default=3000)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hatch_link_times.json"))
    a = ap.parse_args()
    from orip import lib
    if a.lib:
        lib.LIB_PATH = os.path.abspath(a.lib)
    from orip.device import Device
    import hatch_double as HD
    import hatch_link_double as LD
    import occlude_double as OD
    side = int(np.ceil(np.sqrt(a.polygons)))
    inputs = {"polygons": (polygons(a.polygons), 2200 * side + 200), "single": ([[HD.single_polygon(a.edges).astype(np.float64)]], 12000)}
    res = {"polygons": a.polygons, "edges": a.edges, "reps": a.reps, "spacing": SPACING, "inset": INSET, "reach": REACH, "lib": a.lib, "inputs": {}}
    dev = Device(0)
    try:
        for name, (polys, size) in inputs.items():
            table = HD.polys_table(polys)
            fg = np.arange(table.n_sub, dtype=np.int32)
            m = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=1.0, W=size, H=size, invert_y=0)
            t_hatch, t_link, state = [], [], {}

            def prepare():
                dev.svg_flatten(table, 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
                t0 = time.perf_counter()
                st = dev.svg_hatch(fg, 1.0, SPACING, INSET, HD.HORIZONTAL | HD.SERPENTINE)
                t1 = time.perf_counter()
                n_all = table.n_sub + st["segments"]
                off, _ = dev.gcode_to_steps(None, None, m, n=n_all)
                n = len(off) - 1
                if "cls" not in state:
                    src = dev.gcode_steps_source(n)
                    groups = dev.svg_hatch_groups(st["segments"])
                    state.update(cls=np.where(src < table.n_sub, -1, 2 * groups[np.maximum(src - table.n_sub, 0)]).astype(np.int32), n=n, n_all=n_all, hatch=st)
                return t1 - t0

            def link():
                t0 = time.perf_counter()
                out = dev.L.orip_svg_hatch_link(dev.h, state["cls"].ctypes.data, state["n"], fg.ctypes.data, fg.ctypes.data, len(fg), gm, lib.HATCH_LINK_CLAMP, REACH, st8.ctypes.data)
                t1 = time.perf_counter()
                dev._ck(out)
                return t1 - t0

            import ctypes as C
            gm = C.byref(lib.GcodeMap(**{k: m[k] for k, _ in lib.GcodeMap._fields_}))
            st8 = np.zeros(8, np.int64)
            for rep in range(a.reps + 1):
                th = prepare(); tl = link()
                if rep:
                    t_hatch.append(th); t_link.append(tl)
            stats = {k: int(v) for k, v in zip(lib.HATCH_LINK_STATS, st8)}
            r = {"subpaths": int(table.n_sub), "ring_points": int(table.sub_off[-1] + table.n_sub), "strokes": state["n"], "hatch": state["hatch"], "stats": stats,
                 "hatch_s_median": float(np.median(t_hatch)), "link_s_median": float(np.median(t_link)), "link_s_min_max": [float(min(t_link)), float(max(t_link))],
                 "pen_lifts_without": state["n"], "pen_lifts_with": stats["paths_out"]}
            kern = {k: [] for k in PHASES}
            for rep in range(a.reps):
                prepare()
                dev.prof_reset(); dev.prof_enable(True); link(); dev.prof_enable(False)
                for k in kern:
                    kern[k].append(dev.prof_get(k)[0] * 1e-3)
            r["phases_s_median"] = {k: float(np.median(v)) for k, v in kern.items()}
            if stats["lines"] <= a.check_lines and stats["in_reach"] * r["ring_points"] <= 5000000:      # the double tests every pair against every edge
                prepare()
                p_off, p_mm = dev.svg_paths(state["n_all"])
                off, pts = dev.gcode_steps_fetch(state["n"], int(p_off[-1]))
                got = dev.svg_hatch_link(state["cls"], fg, fg, m, True, REACH, n=state["n"])
                r_off, r_pts = OD.rings_to_steps(p_off, p_mm, fg.tolist(), m, True)
                want = LD.hatch_link(off[:state["n"] + 1], pts[:int(off[state["n"]])], state["cls"], r_off, r_pts, fg, REACH)
                r["equals_sequential_definition"] = bool(all(np.array_equal(x, y) for x, y in zip(got[:4], want[:4])) and got[4] == want[4])
            print(f"{name}: hatch call {r['hatch_s_median'] * 1e3:.2f} ms, link call {r['link_s_median'] * 1e3:.2f} ms, {stats['lines']} lines -> {stats['paths_out'] - int(table.n_sub)} "
                  f"zigzags; pen lifts of the whole stream {r['pen_lifts_without']} -> {r['pen_lifts_with']}")
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
