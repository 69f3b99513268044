#!/usr/bin/env python3
"""tests/golden/make_golden_stream.py -- golden vectors for the plotter stream (13_build_stream.py + shared/omnirevolve_plotter_stream_creator_helper.py).

Runs ONLY in the build container (needs /root/reference).  Both reference files are pure Python (the stage imports cv2 only for a fall-back it
does not take: the stand-in of this directory is registered as `cv2`), so every byte recorded here is the reference's own output:
  * bres*      : bresenham_dir_codes on seeded random and degenerate segments
  * travel*    : bytes of travel_ramped for single moves (short / long / odd lengths), default helper Config
  * poly*      : bytes of emit_polyline for random polylines with sharp corners, short and long edges, repeated points, both ramp profiles
  * e2e_{a,b}* : plot_stream.bin / plot_stream.json of 13_build_stream.main() on the ops of golden_e2e_{a,b}.npz, plus a colour-remap variant
  * golden_stream_edges.npz (write_edges): the same two files for a hand-written plot of edge cases, with its ops
  * golden_stream_long.npz (write_long): 52 segments of 46 341 to 200 000 steps and the sha256 of bresenham_dir_codes on each
Nothing from the reference is copied: the fixture holds arrays only.   Usage: python tests/golden/make_golden_stream.py
"""
from __future__ import annotations

import contextlib
import importlib.util
import io
import json
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/image_processor"
sys.path.insert(0, HERE)
import cv2_standin  # noqa: E402

sys.modules["cv2"] = cv2_standin
sys.path.insert(0, REF)
sys.path.insert(0, "/root/reference/shared")
import omnirevolve_plotter_stream_creator_helper as RH  # noqa: E402


def load_ref(fname):
    spec = importlib.util.spec_from_file_location("ref_" + fname[:2], os.path.join(REF, fname))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def main():
    rng = np.random.default_rng(13)
    g = {}
    # ---- bresenham_dir_codes
    segs = [(0, 0, 0, 0), (5, 5, 5, 9), (5, 9, 5, 5), (3, 3, 9, 3), (9, 3, 3, 3), (0, 0, 7, 7), (7, 7, 0, 0), (0, 7, 7, 0), (0, 0, 10, 5), (0, 0, 5, 10), (0, 0, 9, 4), (10, 4, 0, 0)]
    segs += [tuple(int(v) for v in rng.integers(0, 60, 4)) for _ in range(300)] + [tuple(int(v) for v in rng.integers(0, 12000, 4)) for _ in range(40)]
    g["bres_segs"] = np.array(segs, np.int32)
    codes = [np.array(RH.bresenham_dir_codes(*s), np.uint8) for s in segs]
    g["bres_off"] = np.concatenate([[0], np.cumsum([len(c) for c in codes])]).astype(np.int64)
    g["bres_codes"] = np.concatenate(codes)
    # ---- travel_ramped, single moves
    moves = [(0, 0, 1, 0), (0, 0, 2, 1), (0, 0, 3, 3), (10, 10, 10, 490), (0, 0, 479, 0), (0, 0, 480, 7), (0, 0, 481, 100), (5, 5, 2000, 900), (3000, 100, 20, 4000), (0, 0, 0, 7)]
    moves += [tuple(int(v) for v in rng.integers(0, 3000, 4)) for _ in range(12)]
    g["travel_moves"] = np.array(moves, np.int32)
    outs = []
    for m in moves:
        w = RH.StreamWriter(); RH.travel_ramped(w, *m, RH.Config()); outs.append(np.frombuffer(bytes(w.out), np.uint8))
    g["travel_off"] = np.concatenate([[0], np.cumsum([len(o) for o in outs])]).astype(np.int64); g["travel_bytes"] = np.concatenate(outs)
    # ---- emit_polyline
    polys = []
    for i in range(24):
        n = int(rng.integers(2, 30))
        scale = [4, 40, 400, 1500][i % 4]
        p = np.cumsum(rng.integers(-scale, scale + 1, (n, 2)), axis=0) + 4000
        if i % 5 == 0 and n > 4:
            p[3] = p[2]                                  # repeated point: a segment without steps between two corners
        if i % 3 == 0 and n > 5:
            p[4] = p[2]                                  # reversal: a 0-degree corner
        polys.append(np.clip(p, 0, 12000).astype(np.int64))
    polys.append(np.array([[0, 0], [2000, 0], [2000, 1], [0, 1]], np.int64))       # long edges around two sharp corners: full windows
    polys.append(np.array([[0, 0], [100, 0], [0, 0], [100, 0]], np.int64))
    offp = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int64)
    g["poly_off"] = offp; g["poly_pts"] = np.concatenate(polys).astype(np.int32)
    for profile in ("triangle", "scurve"):
        outs = []
        for p in polys:
            w = RH.StreamWriter(); RH.emit_polyline(w, RH.Config(profile=profile, div_start=25, corner_div=30, corner_window_steps=800), [tuple(int(v) for v in q) for q in p])
            outs.append(np.frombuffer(bytes(w.out), np.uint8))
        g[f"poly_{profile}_off"] = np.concatenate([[0], np.cumsum([len(o) for o in outs])]).astype(np.int64)
        g[f"poly_{profile}_bytes"] = np.concatenate(outs) if outs else np.zeros(0, np.uint8)
    # ---- 13_build_stream.main() on the ops of the e2e fixtures
    m13 = load_ref("13_build_stream.py")
    for tag in ("a", "b"):
        G = np.load(os.path.join(HERE, f"golden_e2e_{tag}.npz"))
        cfg = json.loads(bytes(G["cfg_json"]).decode())
        man = json.loads(bytes(G["manifest_json"]).decode())
        layers = {}
        for n in cfg["color_names"]:
            kinds = G[f"ops_kinds_{n}"]; off = G[f"ops_{n}_off"]; pts = G[f"ops_{n}_pts"]
            layers[n] = [{"type": "line", "points": pts[off[i]:off[i + 1]].astype(np.float32)} if k == 0 else {"type": "tap", "x": int(pts[off[i], 0]), "y": int(pts[off[i], 1])}
                         for i, k in enumerate(kinds)]
        for variant, extra, env in (("", {}, {}), ("_remap", {"stream_color_by_order": [3, 0, 1, 2], "stream_color_by_name": {"layer_mid": 5}}, {}),
                                    ("_env", {}, {"STREAM_FORCE_COLOR_INDEX": "6"})):
            g[f"e2e_{tag}{variant}_bin"], g[f"e2e_{tag}{variant}_json"] = run_main(m13, dict(cfg, **extra), man, layers, env)
            g[f"e2e_{tag}{variant}_cfg"] = np.frombuffer(json.dumps(extra).encode(), np.uint8)
    np.savez_compressed(os.path.join(HERE, "golden_stream.npz"), **g)
    print("golden_stream.npz:", len(g), "arrays;", {k: int(v.size) for k, v in g.items() if k.endswith("_bin")})
    write_edges(m13)
    write_long()


LONG_PAIRS = [(70000, 69999), (70000, 35000), (70001, 35000), (99999, 1), (1, 99999), (131072, 65536), (131071, 3), (100000, 50000), (100000, 49999), (65537, 65536),
              (200000, 100000), (46341, 46340), (92682, 46341)]


def long_segments():
    """every (dx, dy) of LONG_PAIRS in the four sign combinations; an axis that rises starts at 0, one that falls at 2^30, so every coordinate lies in 0 .. 2^30.
    Exact ties of the error term (dy = dx / 2), near-diagonals, and 2 (k + 1) minor at or beyond 2^31 on more than half of the steps"""
    A = 1 << 30
    return np.array([(0 if sx > 0 else A, 0 if sy > 0 else A, dx if sx > 0 else A - dx, dy if sy > 0 else A - dy)
                     for dx, dy in LONG_PAIRS for sx in (1, -1) for sy in (1, -1)], np.int32)


def write_long():
    """golden_stream_long.npz: the long segments and the sha256 of each one's bresenham_dir_codes (as uint8 bytes, one code a byte); the codes themselves are 5 MB"""
    import hashlib
    segs = long_segments()
    dig = np.zeros((len(segs), 32), np.uint8); cnt = np.zeros(len(segs), np.int64)
    for i, s in enumerate(segs):
        c = np.array(RH.bresenham_dir_codes(*(int(v) for v in s)), np.uint8)
        cnt[i] = len(c); dig[i] = np.frombuffer(hashlib.sha256(c.tobytes()).digest(), np.uint8)
    np.savez_compressed(os.path.join(HERE, "golden_stream_long.npz"), long_segs=segs, long_steps=cnt, long_sha256=dig)
    print("golden_stream_long.npz:", len(segs), "segments,", int(cnt.sum()), "steps")


def run_main(m13, cfg, man, layers, env):
    """plot_stream.bin / plot_stream.json of the reference's main() on layers {name: ops}, as uint8 arrays"""
    with tempfile.TemporaryDirectory() as td:
        full = dict(cfg); full["output_dir"] = td
        with open(os.path.join(td, "config.json"), "w") as f:
            json.dump(full, f)
        for n, ops in layers.items():
            os.makedirs(os.path.join(td, n), exist_ok=True)
            with open(os.path.join(td, n, "ops.pkl"), "wb") as f:
                pickle.dump(ops, f)
        with open(os.path.join(td, "vector_manifest.json"), "w") as f:
            json.dump(man, f)
        os.environ["CONFIG_PATH"] = os.path.join(td, "config.json")
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                m13.main()
        finally:
            for k, v in old.items():
                if v is None: os.environ.pop(k, None)
                else: os.environ[k] = v
        return tuple(np.frombuffer(open(os.path.join(td, f), "rb").read(), np.uint8) for f in ("plot_stream.bin", "plot_stream.json"))


def edge_layers(W=840, H=1188):
    """a hand-written plot at the places where stage 13's rules are easy to get wrong: an empty layer, an approach to a one-point line that is then
    skipped, taps with and without a travel, a line that starts on the cursor, a repeated point, half-integer rounding, clamping that merges points,
    a one-step travel, a colour byte with no approach"""
    line = lambda *p: {"type": "line", "points": np.array(p, np.float32).reshape(-1, 2)}      # noqa: E731
    tap = lambda x, y: {"type": "tap", "x": x, "y": y}                                        # noqa: E731
    return {"e0": [],
            "e1": [line((50, 60)), tap(50, 60), tap(50, 60), tap(300, 20), line((300, 20), (340, 20), (340, 90)), line((340, 90), (10, 95)),
                   line((10, 95), (10, 95), (12, 95), (12.5, 96.5), (13.5, 97.5))],
            "e2": [tap(14, 98), line((7, 7), (7, 7)), line((-30, -5), (W + 40, 3), (W + 90, H + 7), (5, H + 50)), tap(5, H - 1)],
            "e3": [line((6, H - 1), (6, H - 2)), line((100, 100), (101, 100), (101, 101), (100, 100)), line((400, 400))],
            "e4": []}


def write_edges(m13=None):
    """golden_stream_edges.npz: the reference's main() on edge_layers(); bin, json, cfg, manifest and the ops as arrays (scheme of golden_e2e_*.npz)"""
    m13 = m13 or load_ref("13_build_stream.py")
    layers = edge_layers()
    cfg = {"color_names": list(layers), "pixels_per_mm": json.loads(bytes(np.load(os.path.join(HERE, "golden_e2e_a.npz"))["cfg_json"]).decode())["pixels_per_mm"]}
    man = {"image_size": [840, 1188], "coords": "pixel_top_left",
           "layers": [{"name": n, "color_name": n, "color_index": i + 1, "file": f"{n}/ops.pkl", "count_ops": len(ops)} for i, (n, ops) in enumerate(layers.items())]}
    g = {"cfg_json": np.frombuffer(json.dumps(cfg).encode(), np.uint8), "manifest_json": np.frombuffer(json.dumps(man).encode(), np.uint8)}
    g["bin"], g["json"] = run_main(m13, cfg, man, layers, {})
    for n, ops in layers.items():
        q = [np.asarray(o["points"], np.float32).reshape(-1, 2) if o["type"] == "line" else np.array([[o["x"], o["y"]]], np.float32) for o in ops]
        g[f"ops_kinds_{n}"] = np.array([0 if o["type"] == "line" else 1 for o in ops], np.uint8)
        g[f"ops_{n}_off"] = np.concatenate([[0], np.cumsum([len(v) for v in q])]).astype(np.int64)
        g[f"ops_{n}_pts"] = np.concatenate(q) if q else np.zeros((0, 2), np.float32)
    np.savez_compressed(os.path.join(HERE, "golden_stream_edges.npz"), **g)
    print("golden_stream_edges.npz:", len(g), "arrays;", int(g["bin"].size), "bytes,", bytes(g["json"]).decode())


if __name__ == "__main__":
    main()
