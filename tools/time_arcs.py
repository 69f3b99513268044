"""What --arcs costs (orip/gcode.py, csrc/gcode_arc.hip), on two seeded G-code files: --circles full circles of r = 5 mm (G2 with an I word alone), and
--fillets short fillets (quarter arcs of r = 0.4 mm between the treads of staircases, a hundred to a path).  Per file, after a warm-up, --reps timed runs,
median and spread (min .. max) of the host clock around  flatten + conversion of the resident polylines  (orip_gcode_flatten, orip_gcode_to_steps(NULL,
NULL)), beside the conversion alone on the same points uploaded (orip_gcode_to_steps(off, pts)); the parse on the host and the kernels' own times next to it.
usage: python tools/time_arcs.py [--circles N] [--fillets N] [--reps R] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT)
import numpy as np


def circles_gcode(n, seed=1, r=5.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform([r + 1, r + 1], [209 - r, 296 - r], (n, 2))
    return "G21 G90 G91.1 G17\n" + "".join(f"G0 X{x + r:.3f} Y{y:.3f}\nM3\nG2 I{-r:g}\nM5\n" for x, y in c.tolist())


def fillets_gcode(n, seed=2, per_path=100):
    rng = np.random.default_rng(seed)
    out = ["G21 G17\n"]
    stair = "G1 X0.6\nG3 X0.4 Y0.4 J0.4\nG1 Y0.6\nG2 X0.4 Y0.4 I0.4\n"
    left = n
    while left > 0:
        k = min(left, per_path)
        x, y = rng.uniform([1, 1], [130, 220])
        out.append(f"G90\nG0 X{x:.3f} Y{y:.3f}\nG91\nM3\n" + stair * (k // 2) + ("G1 X0.6\nG3 X0.4 Y0.4 J0.4\n" if k & 1 else "") + "M5\n")
        left -= k
    return "".join(out)


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def measure(dev, name, text, reps):
    from orip import gcode as GC
    o = GC.GcodeOptions(arcs=True)
    tol = GC.arc_tolerance(o)
    W, H = GC.target_size(o)
    m = dict(scale_x=o.scale_x, scale_y=o.scale_y, offset_x_mm=o.offset_x_mm, offset_y_mm=o.offset_y_mm, steps_per_mm=o.steps_per_mm, W=W, H=H, invert_y=0)
    t0 = time.perf_counter(); table, moves = GC.parse_gcode_arcs(text); parse = time.perf_counter() - t0
    n = len(table.sub_off) - 1

    def resident():
        total, st = dev.gcode_flatten(table, tol)
        off, _ = dev.gcode_to_steps(None, None, m, fetch_points=False, n=n)
        return total, st, off
    total, st, off0 = resident()                                            # code objects; every buffer has grown
    off_mm, pts_mm = dev.svg_paths()
    up0, _ = dev.gcode_to_steps(off_mm, pts_mm, m, fetch_points=False)
    assert np.array_equal(off0, up0)
    a, b = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); resident(); a.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); dev.gcode_to_steps(off_mm, pts_mm, m, fetch_points=False); b.append(time.perf_counter() - t0)
    dev.prof_reset(); dev.prof_enable(True); resident(); dev.prof_enable(False)
    kern = {k: dev.prof_get(k)[0] for k in ("k_arc_count", "k_arc_emit")}
    res = {"gcode_bytes": len(text), "paths": n, "segments": len(table.kind), "points": total, "tolerance_mm": tol, "parse_s": parse, "kernel_ms": kern,
           "flatten_and_convert_s": spread(a), "convert_uploaded_s": spread(b), **st}
    print(f"{name}: {st['arcs']} arcs ({st['full_circles']} full circles) in {n} paths -> {st['pieces']} pieces, {total} points within {tol:g} mm; parse {1e3 * parse:.1f} ms on the host")
    for k, v in (("flatten + convert", res["flatten_and_convert_s"]), ("convert, uploaded", res["convert_uploaded_s"])):
        print(f"  {k:18s} median {1e3 * v['median']:8.2f} ms  (min {1e3 * v['min']:.2f}, max {1e3 * v['max']:.2f}; {reps} runs after warm-up)")
    print("  kernel ms:", json.dumps(kern))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circles", type=int, default=10000)
    ap.add_argument("--fillets", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip.device import Device
    dev = Device(0)
    try:
        res = {"reps": a.reps, "circles": measure(dev, "circles", circles_gcode(a.circles), a.reps), "fillets": measure(dev, "fillets", fillets_gcode(a.fillets), a.reps)}
    finally:
        dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
