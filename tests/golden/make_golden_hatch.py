#!/usr/bin/env python3
"""tests/golden/make_golden_hatch.py -- golden vectors for the hatch fill (orip_svg_hatch; stream_generators/plotter_demo/omnirevolve_plotter_demo.py,
hatch_fill :220-260).

Runs ONLY where the reference is (/root/reference).  The demo module is imported with empty stand-ins for what its own imports do not find as shipped
(matplotlib.textpath, matplotlib.font_manager, and xyplotter_stream_creator_helper, the name under which it imports its helper); only hatch_fill is
reached.  hatch_fill is called with a drawer that writes down every travel_to / line_to, and per case the fixture keeps the integer polygons, (spacing,
inset, serpentine) and the recorded segments (x0, y, x1, y) in call order.  Nothing from the reference is copied: the fixture holds arrays only.
time_single_ref_s is the wall time of the reference's hatch_fill on tests/hatch_double.py's single_polygon() at 20 steps spacing (0.5 mm at 40 steps per
mm), for tools/time_hatch.py to quote as context.   Usage: python tests/golden/make_golden_hatch.py [--no-time]
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))

for name in ("matplotlib", "matplotlib.textpath", "matplotlib.font_manager", "xyplotter_stream_creator_helper"):     # empty stand-ins, never called by hatch_fill
    sys.modules[name] = types.ModuleType(name)
sys.modules["matplotlib.textpath"].TextPath = None
sys.modules["matplotlib.font_manager"].FontProperties = lambda **kw: None
for attr in ("Config", "StreamWriter", "travel_ramped"):
    setattr(sys.modules["xyplotter_stream_creator_helper"], attr, None)
spec = importlib.util.spec_from_file_location("ref_plotter_demo", "/root/reference/stream_generators/plotter_demo/omnirevolve_plotter_demo.py")
RD = importlib.util.module_from_spec(spec); sys.modules["ref_plotter_demo"] = RD; spec.loader.exec_module(RD)

import hatch_double as HD


class Recorder:
    """the three calls hatch_fill makes on its drawer"""
    def __init__(self): self.seg, self.at = [], None
    def travel_to(self, x, y): self.at = (x, y)
    def _pen_down(self): pass
    def line_to(self, x, y): self.seg.append((self.at[0], self.at[1], x, y)); self.at = (x, y)


def reference(polys, spacing, inset, serpentine):
    r = Recorder()
    RD.hatch_fill(r, [[(int(x), int(y)) for x, y in p.tolist()] for p in polys], int(spacing), 3, inset=int(inset), serpentine=bool(serpentine))
    return np.array(r.seg, np.int64).reshape(-1, 4)


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.int64)


def comb(teeth, pitch=6, height=90):
    """teeth upright rectangles joined by a bar at the bottom: a line through the teeth crosses 2 * teeth edges"""
    p = [[0, 0]]
    for i in range(teeth):
        x = i * pitch
        p += [[x, height], [x + pitch // 2, height], [x + pitch // 2, 10]] + ([[x + pitch, 10]] if i + 1 < teeth else [])
    p += [[(teeth - 1) * pitch + pitch // 2, 0]]
    return np.array(p, np.int64)


def designed():
    c = {}
    c["hole"] = ([rect(0, 0, 400, 300), rect(100, 80, 300, 220)[::-1]], 20, 3, True)
    c["nested_overlapping"] = ([rect(0, 0, 500, 500), rect(50, 50, 450, 450), rect(100, 100, 400, 400), rect(300, 300, 700, 650)], 7, 3, True)
    c["horizontal_edges_on_lines"] = ([np.array([[0, 0], [200, 0], [200, 40], [120, 40], [120, 80], [200, 80], [200, 120], [0, 120], [0, 80], [60, 80], [60, 40], [0, 40]], np.int64)], 40, 0, True)
    c["vertices_on_lines"] = ([np.array([[0, 0], [100, 40], [200, 0], [300, 80], [200, 160], [100, 120], [0, 160], [40, 80]], np.int64)], 40, 0, False)
    c["negative_coordinates"] = ([np.array([[-900, -700], [-15, -650], [-7, -20], [-400, -5], [-880, -300]], np.int64), rect(-3, -3, 2, 2)], 7, 3, True)
    c["negative_zero_inset"] = ([np.array([[-901, -701], [-14, -651], [-6, -21], [-401, -4]], np.int64)], 7, 0, True)
    c["inset_swallows"] = ([np.array([[0, 0], [300, 0], [150, 400]], np.int64), rect(400, 0, 450, 100)], 20, 27, True)
    c["lower_than_spacing"] = ([rect(0, 320, 500, 350)], 333, 3, True)
    c["between_lines_empty"] = ([rect(0, 341, 500, 355)], 40, 3, True)
    c["islands_empty_lines"] = ([rect(0, 0, 300, 50), rect(0, 171, 300, 230), rect(50, 333, 200, 401)], 20, 3, True)
    c["islands_no_serpentine"] = ([rect(0, 0, 300, 50), rect(0, 171, 300, 230)], 20, 3, False)
    c["two_points"] = ([np.array([[0, 0], [100, 100]], np.int64)], 20, 0, True)
    c["spacing_one"] = ([np.array([[0, 0], [37, 5], [50, 41], [11, 60], [-9, 30]], np.int64)], 1, 3, True)
    c["comb_block"] = ([comb(300)], 40, 0, True)                         # 600 crossings per row: the block sort
    c["comb_segmented"] = ([comb(1200)], 40, 1, True)                    # 2400 crossings per row: beyond the block sort
    return c


EMPTY_BY_DESIGN = {"between_lines_empty", "two_points"}


def random_groups(n=72, seed=20260101):
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(n):
        polys = [HD.star(rng, rng.integers(-2000, 9000), rng.integers(-2000, 9000), rng.integers(30, 1500), int(rng.integers(3, 40))) for _ in range(int(rng.integers(1, 5)))]
        polys = [np.clip(p, -2000, 9000) for p in polys]
        spacing = int((1, 7, 20, 40, 333)[i % 5])
        if spacing == 1:
            polys = [p // 16 for p in polys]                              # a line per step: keep the group small
        inset = int((0, 3, 27)[(i // 5) % 3])
        out[f"random_{i:02d}"] = (polys, spacing, min(inset, 3) if spacing == 1 else inset, bool((i // 15) % 2 == 0))
    return out


def main():
    g, names = {}, []
    cases = dict(designed(), **random_groups())
    total = 0
    for name, (polys, spacing, inset, serp) in cases.items():
        seg = reference(polys, spacing, inset, serp)
        assert (len(seg) == 0) == (name in EMPTY_BY_DESIGN), (name, len(seg))
        assert (seg[:, 1] == seg[:, 3]).all()
        ours, _ = HD.hatch_segments(np.concatenate([[0], np.cumsum([len(p) for p in polys])]), np.concatenate(polys), np.zeros(len(polys), np.int64), spacing, inset,
                                    HD.HORIZONTAL | (HD.SERPENTINE if serp else 0))
        print(f"{name}: {len(polys)} polygons, spacing {spacing}, inset {inset}, serpentine {serp}: {len(seg)} segments, double {'==' if np.array_equal(ours, seg) else '!='} reference", flush=True)
        names.append(name); total += len(seg)
        g[f"{name}_off"] = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int64); g[f"{name}_pts"] = np.concatenate(polys).astype(np.int32)
        g[f"{name}_prm"] = np.array([spacing, inset, int(serp)], np.int64); g[f"{name}_seg"] = seg.astype(np.int32)
    g["names"] = np.frombuffer(json.dumps(names).encode(), np.uint8)
    g["time_single_ref_s"] = np.array([0.0]); g["time_single_prm"] = np.array([100000, 20, 27, 1], np.int64)
    if "--no-time" not in sys.argv:
        poly = HD.single_polygon(100000)
        t0 = time.perf_counter(); seg = reference([poly], 20, 27, True); g["time_single_ref_s"] = np.array([time.perf_counter() - t0])
        g["time_single_segments"] = np.array([len(seg)], np.int64)
        print(f"single polygon of 100000 edges: {len(seg)} segments, reference {g['time_single_ref_s'][0]:.1f} s", flush=True)
    path = os.path.join(HERE, "golden_hatch.npz")
    np.savez_compressed(path, **g)
    print("golden_hatch.npz:", len(names), "cases,", total, "segments,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
