#!/usr/bin/env python3
"""tests/golden/make_golden_gcode.py -- golden vectors for gcode2stream (svg_to_stream/gcode2stream.py + shared/omnirevolve_plotter_stream_creator_helper.py).

Runs ONLY in the build container (needs /root/reference).  Both reference files are pure Python, so every value recorded here is the reference's own:
  * parse_<i>_*   : extract_polylines_mm on G-code texts of our own making that hit every rule of the parser
  * conv_<i>_*    : convert_polylines_to_steps of seeded paths under several option sets (flip, offsets and scales that clamp, exact .5 steps)
  * order_<name>* : order_paths_nearest as index permutations (recovered by object identity) for seeded sets of (first point, last point)
  * main_<i>_*    : the file written by main([...]) for whole command lines
Nothing from the reference is copied: the fixture holds arrays only (texts as uint8, options as JSON bytes).   Usage: python tests/golden/make_golden_gcode.py
"""
from __future__ import annotations

import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/svg_to_stream/gcode2stream.py"
sys.path.insert(0, "/root/reference/shared")
import omnirevolve_plotter_stream_creator_helper as RH  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_gcode2stream", REF)
R = importlib.util.module_from_spec(spec); sys.modules[spec.name] = R; spec.loader.exec_module(R)      # dataclasses look the module up by name


def u8(s) -> np.ndarray:
    return np.frombuffer(s if isinstance(s, bytes) else s.encode("utf-8"), np.uint8)


def flat(paths, dtype):
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    pts = np.asarray([q for p in paths for q in p], dtype).reshape(-1, 2)
    return off, pts


# ---------------------------------------------------------------- texts for the parser
PARSE_TEXTS = [
    # plain square, M3 / M5, both comment forms, an empty and a comment-only line
    "G21 G90 ; metric, absolute\n(a square)\nG0 X10 Y10\nM3\nG1 X20 Y10\nG1 X20 Y20 (corner) \nG1 X10 Y20\n\nG1 X10 Y10\nM5\n;only a comment\nG0 X0 Y0\n",
    # glued words are one word and are skipped whole; lower case letters; bare letters; bad numbers
    "m3\ng1 x5 y5\nG1X10Y20\nG1 X Y7\nG1 X1e1 Y--3\nG1 X12.5abc Y8\nG1 Xnan0 Y9\ng1 x+7.25 y-.5\nM5\n",
    # G91 chains (float64 sums in file order), back to G90
    "G91\nM3\nG1 X0.1 Y0.2\nG1 X0.1 Y0.2\nG1 X0.1\nG1 Y-0.7\nG90\nG1 X3 Y3\nM5\nG91 G1 X1 Y1\nM4\nG1 X-0.3 Y1e-3\n",
    # G20 in mid-line: the X before it is still mm, the Y after it inches; G21 switches back inside a line too
    "M3\nG1 X10 G20 Y1\nG1 X1 Y1\nG1 X2 G21 Y30\nG1 X31 Y30\nM5\n",
    # Z-inferred pen, with and without an M word on the line; Z in inches keeps its sign
    "G1 Z-1\nG1 X5 Y0\nG1 X5 Y5 Z0\nG1 Z0.5\nG1 X9 Y9\nG1 Z-2 M5\nG1 X1 Y1\nG1 Z3 M3\nG1 X2 Y2\nG1 X4 Y2 Z1\nG20\nG1 Z-0.1 X1\nG1 X2 Y1\n",
    # pen down and up again without motion (no path), pen up closing a one-move path, a trailing open path, repeated M3
    "M3\nM5\nM3\nG1 X1 Y1\nM5\nG0 X50 Y50\nM3\nM3\nG1 X60 Y50\nG1 X60 Y50\nG1 X60 Y60\n",
    # comments: unclosed paren eats the rest of the line only, no nesting, a stray closing paren, ';' inside parens cuts first
    "M3 (pen\nG1 X1 Y1 (a (b) X99 Y99\nG1 X2 ) Y2\nG1 X3 (c ; d) Y3\nG1 (x) X4 (y) Y4 (z\nG1 X5 Y5\n",
    # numbers that float() takes: exponents, underscores, inf-free; M codes as floats (M3.9 -> 3); G codes that mean nothing; unknown letters
    "M3.9\nG1.0 X1_0 Y1e0 F1200 S255\nG28\nG2 X5 Y5 I1 J1\nT1 N100 G1 X6 Y6.000000001\nM05\nG1 X7 Y7\nM4.2\nG01 X8 Y8\n",
    # \r\n and \r line ends, tabs, form feed, non-ASCII in comments and a broken UTF-8 byte
    b"M3\r\nG1\tX1\tY1\rG1 X2 Y2 ; caf\xc3\xa9 \xff\nG1 X3\x0cG1 Y3\n(\xe2\x82\xac) G1 X4 Y4\nM5",
    # nothing to draw
    "G21\nG90\nG0 X10 Y10\nG0 X20 Y20\n",
    "",
]


def rec_parse(g):
    for i, t in enumerate(PARSE_TEXTS):
        raw = t if isinstance(t, bytes) else t.encode("utf-8")
        with tempfile.TemporaryDirectory() as td:
            p = Path(td) / "in.gcode"; p.write_bytes(raw)
            paths, moves = R.extract_polylines_mm(p)
        off, pts = flat(paths, np.float64)
        g[f"parse_{i}_text"] = u8(raw); g[f"parse_{i}_off"] = off; g[f"parse_{i}_pts"] = pts; g[f"parse_{i}_moves"] = np.array([moves], np.int64)
    g["parse_count"] = np.array([len(PARSE_TEXTS)], np.int64)


# ---------------------------------------------------------------- conversion to steps
def seeded_paths_mm(rng, n, span, jitter):
    paths = []
    for _ in range(n):
        k = int(rng.integers(2, 9))
        p = rng.uniform(-0.1 * span, 1.1 * span, 2) + np.cumsum(rng.normal(0, jitter, (k, 2)), axis=0)
        if rng.random() < 0.3:
            p[1] = p[0]                                   # a repeated point
        if rng.random() < 0.2:
            p[:] = p[0] + rng.uniform(-0.01, 0.01, (k, 2))   # a path that collapses to one step position
        paths.append([(float(a), float(b)) for a, b in p])
    return paths


CONV_SETS = [   # steps_per_mm, invert_y, W, H, offset_x, offset_y, scale_x, scale_y
    (10.0, False, 2100, 2970, 0.0, 0.0, 1.0, 1.0),
    (10.0, True, 2100, 2970, 0.0, 0.0, 1.0, 1.0),
    (10.0, True, 500, 400, -30.0, 12.5, 1.7, -0.9),     # most points clamp: paths collapse
    (40.0, False, 8400, 11880, 3.3, -7.7, 0.37, 1.01),
    (7.3, True, 1533, 2168, 0.05, 0.05, 25.4, 25.4),
    (10.0, False, 1, 1, 0.0, 0.0, 1.0, 1.0),            # a canvas of one step: everything collapses
]


def rec_conv(g):
    rng = np.random.default_rng(2024)
    paths = seeded_paths_mm(rng, 300, 200.0, 6.0)
    # exact halves in both parities (k + 0.5 steps at 10 steps / mm are k / 10 + 0.05 mm only approximately; use steps_per_mm 2: x.25 mm is exact)
    halves = [[(0.25, 0.75), (1.25, 1.75), (2.25, 0.25)], [(0.75, 0.25), (0.75, 0.75), (1.25, 0.75), (1.75, 1.25)], [(-0.25, -0.75), (0.25, 0.25)],
              [(100.25, 50.75), (100.75, 50.25), (101.25, 50.25)]]
    g["conv_off"], g["conv_pts"] = flat(paths, np.float64)
    g["conv_half_off"], g["conv_half_pts"] = flat(halves, np.float64)
    sets = list(CONV_SETS)
    for i, (spm, inv, W, H, ox, oy, sx, sy) in enumerate(sets):
        out = R.convert_polylines_to_steps(paths, RH.Config(steps_per_mm=spm, invert_y=inv), W, H, ox, oy, sx, sy)
        g[f"conv_{i}_off"], g[f"conv_{i}_out"] = flat(out, np.int64)
    g["conv_sets"] = u8(json.dumps(sets))
    for i, inv in enumerate((False, True)):
        out = R.convert_polylines_to_steps(halves, RH.Config(steps_per_mm=2.0, invert_y=inv), 400, 300, 0.0, 0.0, 1.0, 1.0)
        g[f"conv_half_{i}_off"], g[f"conv_half_{i}_out"] = flat(out, np.int64)


# ---------------------------------------------------------------- order
def order_sets():
    rng = np.random.default_rng(77)
    S = {}
    S["uniform"] = rng.integers(0, 8000, (3000, 4))
    c = rng.integers(0, 8000, (12, 2))
    k = rng.integers(0, 12, 2500)
    S["clustered"] = np.concatenate([(c[k] + rng.integers(-40, 41, (2500, 2))).clip(0), rng.integers(0, 8000, (2500, 2))], 1)
    S["ties"] = np.concatenate([rng.integers(0, 12, (1500, 2)) * 50, rng.integers(0, 12, (1500, 2)) * 50], 1)          # a coarse lattice: many exact ties
    d = rng.integers(0, 3000, (400, 4))
    S["dup_starts"] = np.concatenate([d, np.concatenate([d[:, :2], rng.integers(0, 3000, (400, 2))], 1), d[:200]])
    S["star"] = np.concatenate([np.full((1200, 2), 777), rng.integers(0, 2000, (1200, 2))], 1)                         # one common first point
    S["star_back"] = np.concatenate([np.full((500, 2), 40), np.full((500, 2), 40) + rng.integers(-3, 4, (500, 2))], 1)
    S["row"] = np.stack([rng.integers(0, 9000, 1500), np.full(1500, 5), rng.integers(0, 9000, 1500), rng.integers(0, 9000, 1500)], 1)
    S["column"] = np.stack([np.full(800, 0), rng.integers(0, 9000, 800), rng.integers(0, 50, 800), rng.integers(0, 9000, 800)], 1)
    S["far_cursor"] = np.concatenate([rng.integers(0, 60, (600, 2)), rng.integers(100000, 200000, (600, 2))], 1)       # every last point far outside the first points' box
    S["one"] = np.array([[5, 6, 7, 8]]); S["two"] = np.array([[9, 9, 0, 0], [1, 1, 9, 9]]); S["two_tie"] = np.array([[3, 0, 1, 1], [0, 3, 2, 2]])
    S["large"] = np.concatenate([rng.integers(0, 8400, (20000, 1)), rng.integers(0, 11880, (20000, 1)), rng.integers(0, 8400, (20000, 1)), rng.integers(0, 11880, (20000, 1))], 1)
    return S


def rec_order(g):
    names = []
    for name, e in order_sets().items():
        e = np.asarray(e, np.int64)
        paths = [[(int(a), int(b)), (int(c), int(d))] for a, b, c, d in e]
        t0 = time.time()
        out = R.order_paths_nearest(paths, (0, 0))
        ident = {id(p): i for i, p in enumerate(paths)}
        perm = np.array([ident[id(p)] for p in out], np.int32)
        assert len(perm) == len(paths)
        g[f"order_{name}_ends"] = e.astype(np.int32); g[f"order_{name}_perm"] = perm
        names.append(name)
        print(f"order {name}: {len(paths)} paths, {time.time() - t0:.1f} s", flush=True)
    g["order_names"] = u8(json.dumps(names))


# ---------------------------------------------------------------- whole streams
def drawing(seed=5, n=140, span=180.0):
    """a seeded G-code text: short strokes with sharp and shallow corners, long strokes, some in relative mode, a few outside the sheet"""
    rng = np.random.default_rng(seed)
    out = ["G21", "G90", "M5"]
    for i in range(n):
        k = int(rng.integers(1, 7))
        p0 = rng.uniform(-5, span, 2)
        out.append(f"G0 X{p0[0]:.3f} Y{p0[1]:.3f}")
        out.append("M3" if i % 3 else "G1 Z-1")
        step = [0.4, 3.0, 25.0, 90.0][i % 4]
        if i % 5 == 0:
            out.append("G91")
            for _ in range(k):
                d = rng.normal(0, step, 2)
                out.append(f"G1 X{d[0]:.4f} Y{d[1]:.4f}")
            out.append("G90")
        else:
            p = p0
            for _ in range(k):
                p = p + rng.normal(0, step, 2)
                out.append(f"G1 X{p[0]:.3f} Y{p[1]:.3f} F{int(rng.integers(500, 3000))}")
        out.append("M5" if i % 3 else "G1 Z2")
    return "\n".join(out) + "\n"


TEXT_ORIGIN = "M3\nG1 X30 Y0\nG1 X30 Y30\nM5\nG0 X5 Y5\nM3\nG1 X6 Y5\nM5\n"                      # the first path starts at (0, 0): no first travel
TEXT_COLLAPSE = "G0 X500 Y500\nM3\nG1 X600 Y600\nG1 X700 Y500\nM5\nG0 X-5 Y-5\nM3\nG1 X-9 Y-1\nM5\n"   # everything clamps onto a corner
TEXT_NO_PEN = "G0 X1 Y1\nG1 X5 Y5\n"
SMALL = ["--steps-per-mm", "10"]
MAIN_CASES = [   # (text, arguments)
    ("drawing", SMALL),
    ("drawing", SMALL + ["--no-reorder"]),
    ("drawing", SMALL + ["--invert-y", "1"]),
    ("drawing", SMALL + ["--speed-scale", "0.5"]),
    ("drawing", SMALL + ["--speed-scale", "1.5"]),
    ("drawing", SMALL + ["--speed-scale", "1.0000001"]),
    ("drawing", SMALL + ["--speed-scale", "7"]),                                                  # dividers reach the floor and the constraints bite
    ("drawing", SMALL + ["--profile", "scurve"]),
    ("drawing", SMALL + ["--color-index", "6", "--corner-deg", "120", "--corner-window-steps", "40", "--short-len-steps", "15"]),
    ("drawing", ["--steps-per-mm", "12.5", "--target-width-steps", "1500", "--target-height-steps", "1100", "--offset-x-mm", "-20", "--scale-y", "0.5"]),
    ("drawing", SMALL + ["--target-width-steps", "300"]),                                         # only one size given: the A4 default rules
    ("drawing", SMALL + ["--div-start", "28", "--travel-start-div", "28", "--travel-div-fast", "28", "--div-fast", "20", "--short-div", "22"]),   # the first piece runs at div_start: no speed byte (trap a)
    ("drawing", SMALL + ["--travel-window-steps", "30", "--travel-quant-step", "7", "--div-fast", "9", "--travel-div-fast", "3", "--div-start", "70", "--corner-div", "66"]),  # dividers above 63
    ("drawing2", ["--steps-per-mm", "3", "--scale-x", "1.2", "--offset-y-mm", "4"]),
    ("origin", SMALL),
    ("origin", SMALL + ["--div-start", "28", "--div-fast", "28", "--short-div", "28", "--corner-div", "28"]),   # first piece (a draw segment) at div_start
    ("collapse", SMALL),
    ("no_pen", SMALL),
    ("empty", SMALL),
    ("parse_0", SMALL), ("parse_2", ["--steps-per-mm", "100"]), ("parse_4", SMALL), ("parse_8", SMALL + ["--invert-y", "1"]),
]


def rec_main(g):
    texts = {"drawing": drawing(), "drawing2": drawing(seed=9, n=60, span=400.0), "origin": TEXT_ORIGIN, "collapse": TEXT_COLLAPSE, "no_pen": TEXT_NO_PEN, "empty": ""}
    for i, t in enumerate(PARSE_TEXTS):
        texts[f"parse_{i}"] = t
    used = sorted({c[0] for c in MAIN_CASES})
    for name in used:
        t = texts[name]
        g[f"text_{name}"] = u8(t if isinstance(t, bytes) else t.encode("utf-8"))
    g["main_cases"] = u8(json.dumps(MAIN_CASES))
    for i, (name, args) in enumerate(MAIN_CASES):
        with tempfile.TemporaryDirectory() as td:
            src = Path(td) / "in.gcode"; src.write_bytes(bytes(g[f"text_{name}"]))
            dst = Path(td) / "out.bin"
            with contextlib.redirect_stdout(io.StringIO()):
                R.main([str(src), "-o", str(dst)] + list(args))
            g[f"main_{i}_bin"] = np.frombuffer(dst.read_bytes(), np.uint8)
        print(f"main {i}: {name} {' '.join(args)} -> {g[f'main_{i}_bin'].size} bytes", flush=True)


def main():
    g = {}
    rec_parse(g); rec_conv(g); rec_main(g); rec_order(g)
    path = os.path.join(HERE, "golden_gcode.npz")
    np.savez_compressed(path, **g)
    print("golden_gcode.npz:", len(g), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
