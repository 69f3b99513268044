"""Named inputs of orip_fill_mask: masks of at most 64 x 48 on canvases of at most 300 x 200 (the major coordinate spans up to five blocks of 64 samples),
the placements (3, 1, 4, 3) and (7, 2, 4, 3), six directions, spacings 2 .. 9.  A case is the dict args() unpacks for orip.device.Device.fill_mask and
for tests/fill_double.fill_mask alike."""
import json
import os
import pickle

import numpy as np

STAGES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omnirevolve-image-processor_amd", "stages")

SERPENTINE, ALONG, ACROSS = 1, 2, 4
PLACES = [(3, 1, 4, 3), (7, 2, 4, 3)]
DIRS = [(4096, 0), (0, 4096), (2896, 2896), (3547, 2048), (2048, -3547), (-2048, 3547)]


def case(mask, W, H, place, u, spacing, inset=0, min_len=1, flags=SERPENTINE | ALONG):
    return dict(mask=np.ascontiguousarray(mask, np.uint8), W=W, H=H, place=tuple(place), u=tuple(u), spacing=spacing, inset=inset, min_len=min_len, flags=flags)


def args(c):
    return c["mask"], c["W"], c["H"], c["place"], c["u"], c["spacing"], c["inset"], c["min_len"], c["flags"]


def rect_hole():
    m = np.zeros((30, 40), np.uint8)
    m[4:26, 5:35] = 255
    m[10:18, 14:24] = 0
    return m


def rows_closed_form(c):
    """At u = (4096, 0) and an integer scale s = num (den == 1) the rule has a closed form that needs no sampling: R = 4096 and D = 4096 spacing, so line k is
    the canvas row y = k spacing, im = inset, lm = min_len, and the ink of that row is mask row r = floor((y - dy) / s) with every pixel repeated s times
    from x = dx, cut at the canvas: its runs come from one diff.  -> (seg int32 [n, 4], runs, short)"""
    assert c["u"] == (4096, 0) and c["place"][1] == 1 and c["flags"] & ~SERPENTINE == ALONG
    M, (s, _, dx, dy), W, H = c["mask"] != 0, c["place"], c["W"], c["H"]
    segs, runs, short = [], 0, 0
    for k in range(0, (H - 1) // c["spacing"] + 1):
        y = k * c["spacing"]
        r = (y - dy) // s
        line = np.zeros(W + 2, np.int8)
        if 0 <= r < M.shape[0]:
            x = np.arange(W)
            col = (x - dx) // s
            ok = (col >= 0) & (col < M.shape[1])
            line[1:-1][ok] = M[r, col[ok]]
        d = np.diff(line)
        a0, a1 = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0] - 1
        runs += len(a0)
        keep = (a1 - c["inset"]) - (a0 + c["inset"]) >= c["min_len"]
        short += int((~keep).sum())
        row = [(int(p) + c["inset"], y, int(q) - c["inset"], y) for p, q in zip(a0[keep], a1[keep])]
        if c["flags"] & SERPENTINE and k & 1:
            row = [(x1, y1, x0, y0) for x0, y0, x1, y1 in reversed(row)]
        segs += row
    return np.asarray(segs, np.int32).reshape(-1, 4), runs, short


def cases():
    out = {}
    rh = rect_hole()
    for p, place in enumerate(PLACES):
        for d, u in enumerate(DIRS):
            out[f"rect_hole_p{p}_u{d}"] = case(rh, 300, 200, place, u, 5, inset=1, min_len=3)
    rng = np.random.RandomState(7)
    out["random_60"] = case((rng.rand(48, 64) < 0.6) * 255, 300, 200, PLACES[1], DIRS[3], 4)
    ck = ((np.add.outer(np.arange(48), np.arange(64)) & 1) * 255).astype(np.uint8)
    out["checker_x"] = case(ck, 100, 70, (1, 1, 4, 3), DIRS[0], 2)                         # every run has length 1: all short
    out["checker_y"] = case(ck, 100, 70, (1, 1, 4, 3), DIRS[1], 3)
    out["empty"] = case(np.zeros((48, 64)), 300, 200, PLACES[0], DIRS[3], 4)
    full = np.full((48, 64), 1, np.uint8)                                                 # nonzero is set: not only 255
    for d in (0, 1, 2, 4):                                                                # one run per line, from canvas edge to canvas edge; at 45 degrees
        out[f"full_u{d}"] = case(full, 200, 150, (7, 2, -5, -4), DIRS[d], 9 - d, inset=2, min_len=2)      # the lines leave through the top
    row = np.zeros((8, 64), np.uint8); row[0, 30:41] = 255; row[2, 0:3] = 255; row[4, 63] = 255
    out["run_60_70"] = case(row, 200, 20, (1, 1, 30, 0), DIRS[0], 2)                      # a = 60 .. 70: across the first block boundary
    row = np.zeros((8, 64), np.uint8); row[0, :] = 255; row[2, 1:] = 255; row[4, :63] = 255
    out["run_64_127"] = case(row, 200, 20, (1, 1, 64, 0), DIRS[0], 2)                     # a = 64 .. 127: exactly one block
    out["run_last_block"] = case(row, 200, 20, (1, 1, 194, 0), DIRS[0], 2)                # a = 194 .. 199: in the last, partial block, ended by the canvas
    out["run_into_last_block"] = case(row, 200, 20, (1, 1, 190, 0), DIRS[0], 2, flags=ALONG | ACROSS)
    out["off_canvas"] = case(rh, 90, 60, (3, 1, -20, -10), DIRS[3], 3, inset=1, min_len=2)
    out["off_canvas_y"] = case(rh, 90, 60, (7, 2, -20, -10), DIRS[5], 3, inset=1, min_len=2, flags=SERPENTINE | ALONG | ACROSS)
    out["all_short"] = case(rh, 300, 200, PLACES[0], DIRS[3], 5, inset=200)
    for name, flags in (("along", ALONG), ("across", ACROSS), ("cross", ALONG | ACROSS), ("cross_serpentine", SERPENTINE | ALONG | ACROSS)):
        out[f"family_{name}"] = case(rh, 300, 200, PLACES[1], DIRS[3], 6, inset=1, min_len=3, flags=flags)
    out["negative_k_plain"] = case(rh, 300, 200, PLACES[0], DIRS[2], 5, inset=1, min_len=3, flags=ALONG)      # n.p = 2896 (y - x): k < 0 right of the diagonal
    out["tiny_canvas"] = case(full, 1, 1, (1, 1, 0, 0), DIRS[2], 2)
    return out


# ------------------------------------------------------------------ a synthetic output directory for the stage script
def make_output(tmp_path, fill, outline=True):
    """a 40 x 30 image on a 20 x 15 mm canvas at 10 pixels per mm, two layers, zero margins: what stages 01, 02 and 12 leave"""
    from PIL import Image
    out = tmp_path / "out"; out.mkdir(parents=True)
    names = ["layer_dark", "layer_light"]
    cfg = dict(output_dir=str(out), color_names=names, target_width_mm=20, target_height_mm=15, pixels_per_mm=10, margin_left_mm=0, margin_right_mm=0, margin_top_mm=0,
               margin_bottom_mm=0)
    if fill is not None:
        cfg["fill"] = fill
    (out / "config.json").write_text(json.dumps(cfg))
    Image.fromarray(np.zeros((30, 40, 3), np.uint8)).save(out / "resized.png")
    masks = [np.zeros((30, 40), np.uint8), np.zeros((30, 40), np.uint8)]
    masks[0][5:25, 4:20] = 255; masks[0][10:14, 8:12] = 0
    masks[1][3:28, 24:37] = 255
    layers = []
    for i, name in enumerate(names):
        (out / name).mkdir()
        Image.fromarray(masks[i]).save(out / name / "mask.png")
        ops = [{"type": "line", "points": np.array([[20, 25], [100, 25], [100, 105], [20, 105]], np.float32) + 40 * i}, {"type": "tap", "x": 150, "y": 20 + i}] if outline else []
        with open(out / name / "ops.pkl", "wb") as f:
            pickle.dump(ops, f)
        layers.append({"name": name, "color_name": name, "color_index": i, "file": f"{name}/ops.pkl", "count_ops": len(ops)})
    (out / "vector_manifest.json").write_text(json.dumps({"image_size": [200, 150], "layers": layers, "coords": "pixel_top_left"}, indent=2))
    return out, masks


def snapshot(out):
    return {os.path.relpath(os.path.join(dp, f), out): open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(out) for f in fs}


FILL = {"spacing_mm": 1.0, "angle_deg": 30, "layers": {"layer_dark": {"direction": "cross"}, "layer_light": {"order": "nearest", "spacing_mm": 0.7}}}
