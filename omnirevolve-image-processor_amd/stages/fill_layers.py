# fill_layers.py -- ours, the reference has no such stage: the colour masks of stage 02 are hatched, so that a layer is drawn as tone and not only as its
# outline.  Runs between stages 12 and 13.  For every layer named under the config's fill.layers: <layer>/mask.png + the size of resized.png +
# <layer>/ops.pkl (stage 12's file, read by layer name and never rewritten) -> <layer>/ops_filled.pkl = the outline ops, then the fill ops; the layer's
# entry of vector_manifest.json then names ops_filled.pkl, and stages 13 and 14 follow the manifest.  The hatch itself runs on the GPU through liborip.so
# (include/orip.h: orip_fill_mask states the rule); see orip.stages.fill_options for the config.  Without a `fill` object it writes nothing.  A layer with
# "connect": true has its hatch drawn as zigzags, the links kept on the mask's ink (orip_fill_link): its fill ops are polylines of 2 m points.  A layer with
# "mode": "stipple" is filled with dots on one lattice for the whole canvas, their density following the grey of resized.png inside the mask
# (orip_fill_stipple): its fill ops are taps, and it reports on a [fill-stipple] line.
import json
import os
import sys

import numpy as np

import stage_io as _io
from orip import stages as S
from orip.config import load_config
from orip.lib import FILL_LINK_STATS, FILL_STATS, FILL_STIPPLE_STATS


def outline_end(ops):
    """the canvas point the pen is at behind the outline ops; None when there are none"""
    for op in reversed(ops):
        if op["type"] == "line" and len(op["points"]):
            return tuple(float(v) for v in np.asarray(op["points"]).reshape(-1, 2)[-1])
        if op["type"] == "tap":
            return float(op["x"]), float(op["y"])
    return None


def run(cfg, fill_fn=None, order_fn=None, link_fn=None, stipple_fn=None) -> int:
    """fill_fn / order_fn / link_fn / stipple_fn stand in for the device calls (orip.stages.fill_segments, fill_strokes, fill_dots); None: the GPU"""
    opts = S.fill_options(cfg)
    if opts is None:
        print("[fill] no fill object in the config: nothing written")
        return 0
    out = cfg.output_dir
    base = _io.read_gray(os.path.join(out, "resized.png"))
    if base is None:
        raise SystemExit("Missing resized.png (run step 1 first).")
    h, w = base.shape[:2]
    man_path = os.path.join(out, "vector_manifest.json")
    if not os.path.exists(man_path):
        raise SystemExit(f"Missing manifest: {man_path} (run step 12 first).")
    with open(man_path, "r", encoding="utf-8") as f:
        man = json.load(f)
    entries = {str(e.get("color_name", e.get("name"))): e for e in man.get("layers", [])}
    for name, o in opts.items():
        layer_dir = os.path.join(out, name)
        mask = _io.read_gray(os.path.join(layer_dir, "mask.png"))
        p_ops = os.path.join(layer_dir, "ops.pkl")
        if mask is None or not os.path.exists(p_ops) or name not in entries:
            raise SystemExit(f"Missing mask.png, ops.pkl or manifest entry of {name} (run steps 2 and 12 first).")
        if mask.shape != (h, w):
            raise SystemExit(f"{name}/mask.png is {mask.shape[1]} x {mask.shape[0]}, resized.png {w} x {h}")
        ops = _io.load_pickle(p_ops)
        p_out = os.path.join(layer_dir, "ops_filled.pkl")
        if o.get("mode") == "stipple":                                                # dots whose density follows resized.png inside the mask (include/orip.h: orip_fill_stipple)
            xy, st = S.fill_dots(mask, base, w, h, cfg, o, start=outline_end(ops), stipple_fn=stipple_fn, order_fn=order_fn)
            filled = list(ops) + S.fill_dot_ops(xy)
            _io.save_pickle(p_out, filled)
            entries[name]["file"] = os.path.relpath(p_out, out)
            entries[name]["count_ops"] = len(filled)
            clear_rad, tone_rad = S.fill_stipple_radii(cfg, o, w, h)
            print(f"[fill-stipple] {name}: pitch={o['lattice'][0]} row={o['lattice'][1]} shift={o['lattice'][2]} clear={clear_rad} "
                  f"tone_radius={tone_rad} tone={'on' if o['tone'] else 'off'} lo={o['lo']} hi={o['hi']} order={o['order']} " + " ".join(f"{k}={st[k]}" for k in FILL_STIPPLE_STATS))
            continue
        lst = None
        if "reach" in o:                                                              # connect: the hatch as zigzags (include/orip.h: orip_fill_link)
            strokes, st, lst = S.fill_strokes(mask, w, h, cfg, o, start=outline_end(ops), fill_fn=fill_fn, link_fn=link_fn, order_fn=order_fn)
            filled = list(ops) + S.fill_stroke_ops(strokes)
        else:
            seg, st = S.fill_segments(mask, w, h, cfg, o, start=outline_end(ops), fill_fn=fill_fn, order_fn=order_fn)
            filled = list(ops) + S.fill_ops(seg)
        _io.save_pickle(p_out, filled)
        entries[name]["file"] = os.path.relpath(p_out, out)
        entries[name]["count_ops"] = len(filled)
        print(f"[fill] {name}: angle={o['angle_deg']:.3f} order={o['order']} " + " ".join(f"{k}={st[k]}" for k in FILL_STATS))
        if lst is not None:
            print(f"[fill-link] {name}: reach={o['reach']} " + " ".join(f"{k}={lst[k]}" for k in FILL_LINK_STATS))
    with open(man_path, "w", encoding="utf-8") as f:
        json.dump(man, f, ensure_ascii=False, indent=2)
    print(f"[fill] manifest saved: {man_path}")
    return 0


if __name__ == "__main__":
    sys.exit(run(load_config()))
