"""In-process stage functions with the reference's per-stage inputs / outputs:

    extract_colors(bgr, cfg)            -> {name: mask u8[H,W]}, palette            (02_color_extract.py main)
    detect_edges(masks, cfg)            -> {name: edges u8[H,W]}                   (03_edge_detect.py process_color)
    find_contours(edges, cfg)           -> {name: [int32 (N,1,2)]}                 (04_find_contours.py vectorize_layer)
    scale_vectors / sort_contours / dedup_layer / dedup_cross / plot_order         (05, 07, 08, 10, 12)
    run_path(bgr, cfg)                  -> ops per layer, everything resident on the GPU between stages
    fill_options(cfg) / fill_layer(mask, w, h, cfg, opts)    -> hatch ops of a colour mask                (fill_layers.py; ours)
    fill_strokes(mask, w, h, cfg, opts)                      -> the same hatch as zigzags, links on ink   (fill_layers.py with connect; ours)
    fill_dots(mask, tone, w, h, cfg, opts)                   -> dots whose density follows the tone       (fill_layers.py with mode stipple; ours)

Every function drives liborip.so through orip.device.Device; arrays cross the host boundary only where the
reference's stage API puts a file.
"""
from __future__ import annotations

import math
import threading
from typing import Dict, List, Sequence, Tuple

import os

import numpy as np

from . import lib as _l
from .config import Config, canvas_size_px, margins_px, scale_factors
from .device import Device

_dev: Device | None = None


def device(device_id: int = 0) -> Device:
    global _dev
    if _dev is None:
        _dev = Device(device_id)
    return _dev


# ---------------------------------------------------------------- naming rules of the reference
def darkness_rank02(name: str) -> int:  # 02:17-23
    s = name.lower()
    if "dark" in s: return 0
    if "mid" in s: return 1
    if "skin" in s: return 2
    if "light" in s: return 3
    return 2


def darkness_rank10(name: str) -> int:  # 10:206-208
    order = ["layer_dark", "layer_mid", "layer_skin", "layer_light"]
    return order.index(name) if name in order else 999


def color_index12(name: str) -> int:  # 12:210-219
    if "dark" in name: return 3
    if "skin" in name: return 0
    if "mid" in name: return 1
    if "light" in name: return 2
    return 0


def cluster_names(cfg: Config) -> List[str]:
    """i-th darkest cluster <-> i-th name of sorted(names, key=_darkness_rank) (02:130-133); device layer l = cluster l."""
    return sorted(list(cfg.color_names), key=darkness_rank02)


SUBSAMPLE_LIMIT = 200_000                                    # 02:39
_SUBSAMPLE_MEMO: Dict[Tuple[int, int], np.ndarray] = {}      # (n, limit) -> indices, oldest first
_SUBSAMPLE_MEMO_MAX = 4
_subsample_lock = threading.Lock()


def subsample_indices(n: int, limit: int = 200_000):  # 02:39-44
    """The fixed-seed subsample: a function of (n, limit) alone, and 8-13 ms of host time at 4096^2, so the last few are kept.  The array that comes back
    is shared between callers and read-only."""
    n, limit = int(n), int(limit)
    if n <= limit:
        return None
    with _subsample_lock:
        idx = _SUBSAMPLE_MEMO.get((n, limit))
        if idx is None:
            idx = np.random.default_rng(42).choice(n, size=limit, replace=False)
            idx.setflags(write=False)
            while len(_SUBSAMPLE_MEMO) >= _SUBSAMPLE_MEMO_MAX:
                del _SUBSAMPLE_MEMO[next(iter(_SUBSAMPLE_MEMO))]
            _SUBSAMPLE_MEMO[(n, limit)] = idx
        return idx


def ensure_odd(n: int) -> int:  # 03:9-11
    n = max(3, int(n))
    return n if n % 2 == 1 else n + 1


def lab8_to_bgr(lab_u8) -> Tuple[int, int, int]:
    """_lab_to_bgr (02:58-61), the palette's approx_bgr: 8-bit Lab (L*255/100, a+128, b+128) -> BGR.  Host arithmetic on K triples
    (a by-product for the previews): CIE L*a*b* -> XYZ (D65 white 0.950456 / 1 / 1.088754) -> linear sRGB -> gamma.
    cv2 is not available to pin the last bit (parity unpinned); tests check it against the oracle's forward Lab tables."""
    L = float(lab_u8[0]) * 100.0 / 255.0
    fy = (L + 16.0) / 116.0
    f = (fy + (float(lab_u8[1]) - 128.0) / 500.0, fy, fy - (float(lab_u8[2]) - 128.0) / 200.0)
    xyz = []
    for t, white in zip(f, (0.950456, 1.0, 1.088754)):
        cube = t * t * t
        xyz.append(white * (cube if cube > 0.008856 else (t - 16.0 / 116.0) / 7.787))
    X, Y, Z = xyz
    out = []
    for m in ((0.055648, -0.204043, 1.057311), (-0.969256, 1.875991, 0.041556), (3.240479, -1.53715, -0.498535)):   # B, G, R rows
        c = m[0] * X + m[1] * Y + m[2] * Z
        c = 12.92 * c if c <= 0.0031308 else 1.055 * (max(c, 0.0) ** (1.0 / 2.4)) - 0.055
        out.append(int(min(255, max(0, round(c * 255.0)))))
    return out[0], out[1], out[2]


# ---------------------------------------------------------------- derived parameter blocks
def params08(cfg: Config) -> _l.Params08:  # 08:484-509
    pen_diam = float(cfg.pen_width_px); pen_radius = float(cfg.pen_radius_px)
    W, H = canvas_size_px(cfg)
    col_rad = float(cfg.collision_radius_intra_px)
    post_brush = 16
    return _l.Params08(tap_diam=pen_diam, tap_max_dim=float(cfg.tap_max_dim), min_keep=max(10.0, pen_radius * 0.4),
                       tap_max_per=float(cfg.tap_max_perimeter), tap_max_v=50, sample_step=float(cfg.dedup_sample_step),
                       tail_len_px=float(cfg.ignore_tail_points_intra), col_rad=col_rad, grid_stride=float(cfg.hash_stride_px),
                       max_jump=float(cfg.max_join_jump_px), post_on=1, post_brush=post_brush, post_step=6.0,
                       post_eps=max(1.0, 0.08 * post_brush), post_minlen=max(2 * post_brush, 12), W=W, H=H,
                       brush_forbid=max(1, int(round(2.0 * col_rad))))


def params10(cfg: Config) -> _l.Params10:  # 10:217-229
    pen_diam = float(cfg.pen_width_px); W, H = canvas_size_px(cfg)
    return _l.Params10(tap_diam=pen_diam, min_keep=max(10.0, (pen_diam / 2.0) * 0.4), tap_max_per=2.5 * pen_diam, tap_max_v=50,
                       max_jump=float(cfg.max_join_jump_px), D_lines=pen_diam * 2.0, D_taps=pen_diam * 2.0, step_px=1.0, W=W, H=H)


def r_insert12(cfg: Config) -> float:  # 12:197
    return float(max(80.0, cfg.pen_width_px))


# ---------------------------------------------------------------- stage functions (host arrays in / out)
def resized_size(h: int, w: int, max_dimension: int):
    """01:12-18 -- None when the longest side already fits, else (new_w, new_h) with Python's float scale and int() truncation"""
    m = max(h, w)
    if m <= max_dimension:
        return None
    scale = max_dimension / m
    return int(w * scale), int(h * scale)


def resize_if_needed(img: np.ndarray, cfg: Config, dev: Device | None = None, as_image: bool = False) -> np.ndarray:
    """01 resize_if_needed (:7-23): the image itself when it fits, else its INTER_AREA shrink; as_image also leaves it resident for stage 02"""
    size = resized_size(img.shape[0], img.shape[1], int(cfg.max_dimension))
    if size is None:
        return img
    return (dev or device()).resize_area(img, size[0], size[1], as_image=as_image)


def extract_colors(bgr: np.ndarray, cfg: Config, centers: np.ndarray | None = None, dev: Device | None = None):
    """02 main(), k-means mode.  Returns (masks {name: u8[H,W]}, info) with info = centres (dark->light), counts, labels."""
    d = dev or device()
    names = list(cfg.color_names)
    K = max(2, len(names))
    d.set_image(bgr)
    if centers is None:
        centers, _ = d.kmeans_fit_subsampled(SUBSAMPLE_LIMIT, K)
    cs, counts = d.extract_layers(np.asarray(centers, np.float32))
    masks = {n: d.get_mask(l) for l, n in enumerate(cluster_names(cfg)[:K])}
    return masks, {"centers_lab": cs, "counts": counts, "centers_fit": np.asarray(centers, np.float32)}


def detect_edges(masks: Dict[str, np.ndarray], cfg: Config, dev: Device | None = None) -> Dict[str, np.ndarray]:
    d = dev or device()
    names = list(masks.keys())
    d.set_masks(np.stack([masks[n] for n in names]))
    _detect_edges_resident(d, cfg)
    return {n: d.get_edges(l) for l, n in enumerate(names)}


def _detect_edges_resident(d: Device, cfg: Config):
    d.detect_edges(max(1, int(cfg.edge_morph_kernel)), int(cfg.edge_morph_open_iters), int(cfg.edge_morph_close_iters),
                   ensure_odd(cfg.edge_kernel_size), int(math.floor(cfg.edge_low_threshold)), int(math.floor(cfg.edge_high_threshold)))


def find_contours(edges: Dict[str, np.ndarray], cfg: Config | None = None, dev: Device | None = None) -> Dict[str, List[np.ndarray]]:
    d = dev or device()
    names = list(edges.keys())
    d.set_edges(np.stack([edges[n] for n in names]))
    d.find_contours()
    return {n: d.get_polys(_l.SLOT_CONTOURS, l) for l, n in enumerate(names)}


def scale_vectors(contours: Sequence[np.ndarray], w_src: int, h_src: int, cfg: Config, dev: Device | None = None, layer: int = 0):
    d = dev or device()
    d.set_polys(_l.SLOT_CONTOURS, layer, contours)
    sx, sy, dx, dy = scale_factors(cfg, w_src, h_src)
    d.scale_vectors(layer, sx, sy, dx, dy)
    return d.get_polys(_l.SLOT_SCALED, layer)


def sort_contours(contours: Sequence[np.ndarray], dev: Device | None = None, layer: int = 0):
    d = dev or device()
    d.set_polys(_l.SLOT_SCALED, layer, contours)
    d.sort_contours(layer)
    return d.get_polys(_l.SLOT_SORTED, layer)


def dedup_layer(contours_sorted: Sequence[np.ndarray], cfg: Config, dev: Device | None = None, layer: int = 0):
    d = dev or device()
    d.set_polys(_l.SLOT_SORTED, layer, contours_sorted)
    d.dedup_layer(layer, params08(cfg))
    return d.get_polys(_l.SLOT_LINES_INTRA, layer), d.get_taps(_l.TAPS_INTRA, layer)


def dedup_cross(intra: Dict[str, Tuple[Sequence[np.ndarray], Sequence[Tuple[int, int]]]], cfg: Config, dev: Device | None = None):
    d = dev or device()
    names = list(cfg.color_names)
    for l, n in enumerate(names):
        lines, taps = intra.get(n, ([], []))
        d.set_polys(_l.SLOT_LINES_INTRA, l, lines)
        d.set_taps(_l.TAPS_INTRA, l, taps)
    order = sorted(range(len(names)), key=lambda l: darkness_rank10(names[l]))
    d.dedup_cross(order, params10(cfg))
    return {n: (d.get_polys(_l.SLOT_LINES_CROSS, l), d.get_taps(_l.TAPS_CROSS, l)) for l, n in enumerate(names)}


# ---- previews 06 / 09 / 11 (visual QA; parity unpinned: include/orip.h orip_preview_cover says what is drawn instead of cv2.LINE_AA) ----
def preview_cover(polys: Sequence[np.ndarray], taps: Sequence[Tuple[int, int]], size: Tuple[int, int], thickness: int, radius: int, antialias: bool,
                  dev: Device | None = None, layer: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Coverage planes (lines, taps), uint8 (H, W), of one layer's polylines and taps on the full canvas `size` = (W, H)."""
    d = dev or device()
    d.set_polys(_l.SLOT_LINES_CROSS, layer, polys)
    d.set_taps(_l.TAPS_CROSS, layer, taps)
    return d.preview_cover(_l.SLOT_LINES_CROSS, layer, _l.TAPS_CROSS, size[0], size[1], max(1, int(thickness)), max(0, int(radius)), bool(antialias))


def preview_compose(img: np.ndarray, cover: np.ndarray, bgr) -> np.ndarray:
    """`bgr` laid over img (H, W, 3) uint8 at coverage `cover` (H, W) uint8: (img (255 - A) + colour A + 127) // 255 per channel."""
    A = cover.astype(np.int32)[:, :, None]
    col = np.asarray(bgr, np.int32).reshape(1, 1, 3)
    return ((img.astype(np.int32) * (255 - A) + col * A + 127) // 255).astype(np.uint8)


def preview_images(polys, taps, size, thickness: int, radius: int, antialias: bool, color, tap_color_layer=(0, 0, 255), dev: Device | None = None):
    """One layer of a preview stage: (layer image, colour image) as 09:103-118 builds them -- black lines and `tap_color_layer` discs on white for
    <layer>/preview_*.png, lines and discs in the layer's colour for the composite (06 has no taps: pass [])."""
    cov_l, cov_t = preview_cover(polys, taps, size, thickness, radius, antialias, dev)
    white = np.full((size[1], size[0], 3), 255, np.uint8)
    lay = preview_compose(preview_compose(white, cov_l, (0, 0, 0)), cov_t, tap_color_layer)
    col = preview_compose(preview_compose(white, cov_l, color), cov_t, color)
    return lay, col


def preview_palette(cfg: Config) -> Dict[str, Tuple[int, int, int]]:
    """_load_palette_by_name (06:46-62) / _palette (09:27-42): approx_bgr of palette_by_name.json, else cfg.colors[i]."""
    import json
    import os
    data = None
    path = os.path.join(cfg.output_dir, "palette_by_name.json")
    if os.path.exists(path):
        try:
            with open(path, "r", encoding="utf-8") as f:
                data = json.load(f)
        except Exception:
            data = None
    out = {}
    for i, n in enumerate(cfg.color_names):
        if data and n in data and "approx_bgr" in data[n]:
            b, g, r = data[n]["approx_bgr"]
        else:
            b, g, r = cfg.colors[i]
        out[n] = (int(b), int(g), int(r))
    return out


def ops_from_device(d: Device, layer: int, R: float) -> List[dict]:
    raw = d.plot_order(layer, R)
    lines = d.get_polys(_l.SLOT_LINES_CROSS, layer) if len(raw) else []
    ops = []
    for t, idx, flip, x, y in raw:
        if t == 0:
            p = np.asarray(lines[idx]).reshape(-1, 2).astype(np.float32)
            ops.append({"type": "line", "points": p[::-1].copy() if flip else p})
        else:
            ops.append({"type": "tap", "x": int(x), "y": int(y)})
    return ops


def plot_order(lines: Sequence[np.ndarray], taps: Sequence[Tuple[int, int]], cfg: Config, dev: Device | None = None, layer: int = 0) -> List[dict]:
    d = dev or device()
    d.set_polys(_l.SLOT_LINES_CROSS, layer, lines)
    d.set_taps(_l.TAPS_CROSS, layer, taps)
    return ops_from_device(d, layer, r_insert12(cfg))


# ---------------------------------------------------------------- fill_layers: the colour masks hatched (ours; include/orip.h: orip_fill_mask)
FILL_DEFAULTS = {"spacing_mm": 1.0, "angle_deg": 45.0, "direction": "along", "inset_mm": 0.3, "min_run_mm": 0.5, "serpentine": True, "order": "serpentine"}
FILL_DIRECTIONS = {"along": _l.FILL_ALONG, "across": _l.FILL_ACROSS, "cross": _l.FILL_ALONG | _l.FILL_ACROSS}
FILL_ORDERS = ("serpentine", "nearest")
FILL_CONNECT_KEYS = ("connect", "connect_mm")                                             # fill connect (include/orip.h: orip_fill_link); connect_mm defaults to twice the layer's spacing_mm
# fill stipple (include/orip.h: orip_fill_stipple): a layer, or the fill object for all of them, says "mode": "stipple"; the keys of this table are read only
# there, and inset_mm, serpentine and order are shared with the hatch.  tone_radius_mm has no fixed default: half the layer's stipple_mm
FILL_MODES = ("hatch", "stipple")
FILL_STIPPLE_DEFAULTS = {"stipple_mm": 1.0, "stipple_pattern": "stagger", "tone": True, "tone_lo": 0, "tone_hi": 255}
FILL_STIPPLE_KEYS = ("mode", "tone_radius_mm") + tuple(FILL_STIPPLE_DEFAULTS)
FILL_HATCH_ONLY_KEYS = ("spacing_mm", "angle_deg", "direction", "min_run_mm") + FILL_CONNECT_KEYS      # an error in a stipple layer's own object


def _fill_pixels(what: str, mm, ppm: int, lo: int) -> int:
    if isinstance(mm, bool) or not isinstance(mm, (int, float)) or not math.isfinite(mm):
        raise ValueError(f"fill: {what} must be a number, not {mm!r}")
    px = int(round(float(mm) * ppm))
    if px < lo or px > _l.FILL_LEN_MAX:
        raise ValueError(f"fill: {what} {mm:g} is {px} pixels at {ppm} pixels per mm: {lo} .. 2^15")
    return px


def _fill_stipple_options(name: str, own: dict, o: dict, ppm: int) -> dict:
    """the entry of a layer whose mode is "stipple": own = the layer's own object, o = the same over the fill object over the defaults"""
    from .svg import STIPPLE_PATTERNS, stipple_lattice
    for k in own:
        if k in FILL_HATCH_ONLY_KEYS:                                                 # inherited from the fill object they are ignored: one global hatch setting, one stippled layer
            raise ValueError(f"fill: {k} in layers.{name} belongs to the hatch, and the layer's mode is stipple")
    o = dict(FILL_STIPPLE_DEFAULTS, **o)
    if o["order"] not in FILL_ORDERS:
        raise ValueError(f"fill: order {o['order']!r}: one of " + ", ".join(FILL_ORDERS))
    if not isinstance(o["serpentine"], bool):
        raise ValueError(f"fill: serpentine must be true or false, not {o['serpentine']!r}")
    if not isinstance(o["tone"], bool):
        raise ValueError(f"fill: tone must be true or false, not {o['tone']!r}")
    if o["stipple_pattern"] not in STIPPLE_PATTERNS:
        raise ValueError(f"fill: stipple_pattern {o['stipple_pattern']!r}: one of " + ", ".join(STIPPLE_PATTERNS))
    for k in ("tone_lo", "tone_hi"):
        if isinstance(o[k], bool) or not isinstance(o[k], int) or not 0 <= o[k] <= 255:
            raise ValueError(f"fill: {k} must be an integer in 0 .. 255, not {o[k]!r}")
    if o["tone_lo"] >= o["tone_hi"]:
        raise ValueError(f"fill: tone_lo {o['tone_lo']} must be below tone_hi {o['tone_hi']}")
    pitch = _fill_pixels("stipple_mm", o["stipple_mm"], ppm, 2)
    stated = "tone_radius_mm" in o
    return {"mode": "stipple", "lattice": stipple_lattice(pitch, o["stipple_pattern"]), "inset": _fill_pixels("inset_mm", o["inset_mm"], ppm, 0), "tone": o["tone"],
            "lo": o["tone_lo"], "hi": o["tone_hi"], "tone_radius": _fill_pixels("tone_radius_mm", o["tone_radius_mm"] if stated else 0.5 * o["stipple_mm"], ppm, 0),
            "tone_radius_stated": stated, "flags": _l.FILL_STIPPLE_SERPENTINE if o["serpentine"] else 0, "order": o["order"]}


def fill_options(cfg: Config):
    """the `fill` object of the config file (cfg._raw: Config has no such field) -> None without one, else {layer name: options} for the layers named under
    "layers", in color_names order.  Options: spacing, inset, min_len (pixels: int(round(mm * pixels_per_mm))), u (orip.svg.hatch_direction_vector of
    angle_deg, in the manifest's frame: x right, y down), flags (lib.FILL_*), order ("serpentine": as the device emits; "nearest": greedy from the end of
    the outline), angle_deg; and ONLY with "connect": true the key reach (pixels of connect_mm, default twice the layer's spacing_mm, 1 .. 2^15), which
    makes fill_layers draw the layer's hatch as zigzags (fill_strokes).  A layer whose object, or the fill object, says "mode": "stipple" is filled with dots
    (fill_dots; include/orip.h: orip_fill_stipple) and its entry is another: mode = "stipple", lattice = orip.svg.stipple_lattice of stipple_mm in pixels (2 ..
    2^15) and stipple_pattern ("stagger" / "square"), inset (pixels of inset_mm), tone (false: the plain stipple), lo / hi (tone_lo / tone_hi, darkness = 255 -
    grey: no dots at lo and below, all at hi and above), tone_radius (pixels of tone_radius_mm, default half of stipple_mm) with tone_radius_stated, flags
    (lib.FILL_STIPPLE_SERPENTINE from serpentine), order.  A hatch-only key (FILL_HATCH_ONLY_KEYS) in a stipple layer's own object is an error; inherited from
    the fill object it is ignored.  The FILL_STIPPLE_KEYS are read only where the mode is stipple.  An unknown key, a layer that is not in color_names or a value out of range raises ValueError naming it."""
    from .svg import hatch_direction_vector
    raw = (getattr(cfg, "_raw", None) or {}).get("fill")
    if raw is None:
        return None
    if not isinstance(raw, dict):
        raise ValueError("fill: must be an object")
    for k in raw:
        if k != "layers" and k not in FILL_DEFAULTS and k not in FILL_CONNECT_KEYS and k not in FILL_STIPPLE_KEYS:
            raise ValueError(f"fill: unknown key {k!r}")
    layers = raw.get("layers", {})
    if not isinstance(layers, dict):
        raise ValueError("fill: layers must be an object of layer name -> options")
    for name in layers:
        if name not in cfg.color_names:
            raise ValueError(f"fill: layer {name!r} is not in color_names {list(cfg.color_names)}")
    ppm = int(cfg.pixels_per_mm)
    out = {}
    for name in cfg.color_names:
        if name not in layers:
            continue
        own = layers[name]
        if not isinstance(own, dict):
            raise ValueError(f"fill: layers.{name} must be an object")
        for k in own:
            if k not in FILL_DEFAULTS and k not in FILL_CONNECT_KEYS and k not in FILL_STIPPLE_KEYS:
                raise ValueError(f"fill: unknown key {k!r} in layers.{name}")
        o = dict(FILL_DEFAULTS, **{k: v for k, v in raw.items() if k != "layers"})
        o.update(own)
        mode = o.get("mode", "hatch")
        if mode not in FILL_MODES:
            raise ValueError(f"fill: mode {mode!r}: one of " + ", ".join(FILL_MODES))
        if mode == "stipple":                                                         # the stipple keys are read only here
            out[name] = _fill_stipple_options(name, own, o, ppm)
            continue
        if o["direction"] not in FILL_DIRECTIONS:
            raise ValueError(f"fill: direction {o['direction']!r}: one of " + ", ".join(FILL_DIRECTIONS))
        if o["order"] not in FILL_ORDERS:
            raise ValueError(f"fill: order {o['order']!r}: one of " + ", ".join(FILL_ORDERS))
        if not isinstance(o["serpentine"], bool):
            raise ValueError(f"fill: serpentine must be true or false, not {o['serpentine']!r}")
        if isinstance(o["angle_deg"], bool) or not isinstance(o["angle_deg"], (int, float)) or not math.isfinite(o["angle_deg"]):
            raise ValueError(f"fill: angle_deg must be a finite number, not {o['angle_deg']!r}")
        u = hatch_direction_vector(o["angle_deg"])
        out[name] = {"spacing": _fill_pixels("spacing_mm", o["spacing_mm"], ppm, 2), "inset": _fill_pixels("inset_mm", o["inset_mm"], ppm, 0),
                     "min_len": _fill_pixels("min_run_mm", o["min_run_mm"], ppm, 1), "u": u,
                     "flags": FILL_DIRECTIONS[o["direction"]] | (_l.FILL_SERPENTINE if o["serpentine"] else 0), "order": o["order"],
                     "angle_deg": math.degrees(math.atan2(u[1], u[0]))}
        connect = o.get("connect", False)
        if not isinstance(connect, bool):
            raise ValueError(f"fill: connect must be true or false, not {connect!r}")
        if connect:                                                                   # connect_mm is read only here
            out[name]["reach"] = _fill_pixels("connect_mm", o["connect_mm"] if "connect_mm" in o else 2 * o["spacing_mm"], ppm, 1)
    return out


def fill_placement(cfg: Config, w_src: int, h_src: int) -> Tuple[int, int, int, int]:
    """(num, den, dx, dy) of orip_fill_mask: stage 05's scale (orip.config.scale_factors) as the exact rational, and its offset"""
    w_full, h_full = canvas_size_px(cfg)
    ml, mr, mt, mb = margins_px(cfg)
    inner_w, inner_h = max(1, w_full - ml - mr), max(1, h_full - mt - mb)
    num, den = (inner_w, int(w_src)) if inner_w * int(h_src) <= inner_h * int(w_src) else (inner_h, int(h_src))
    return num, den, ml, mt


def fill_segments(mask, w_src: int, h_src: int, cfg: Config, opts: dict, dev: Device | None = None, layer: int = 0, start=None, fill_fn=None, order_fn=None):
    """the hatch of one layer -> (seg int32 [n, 4] = x0 y0 x1 y1 in canvas pixels, in drawing order, {lib.FILL_STATS}).  mask u8 [h_src, w_src], or None for
    the resident mask of `layer`; opts: one entry of fill_options; start: the canvas point (x, y) the pen comes from, for order "nearest" (None: the
    origin).  fill_fn / order_fn stand in for Device.fill_mask / Device.gcode_order_pens (the CPU tests pass their doubles)."""
    from .stream import to_steps
    if mask is not None and tuple(np.asarray(mask).shape) != (int(h_src), int(w_src)):
        raise ValueError(f"mask of shape {np.asarray(mask).shape} for a source of {w_src} x {h_src}")
    W, H = canvas_size_px(cfg)
    if fill_fn is None:
        d = dev or device()
        fill_fn = lambda *a: d.fill_mask(*a, layer=layer)
    seg, st = fill_fn(mask, W, H, fill_placement(cfg, w_src, h_src), opts["u"], opts["spacing"], opts["inset"], opts["min_len"], opts["flags"])
    seg = np.asarray(seg, np.int32).reshape(-1, 4)
    if opts["order"] == "nearest" and len(seg):
        if order_fn is None:
            order_fn = (dev or device()).gcode_order_pens
        ends = np.concatenate([to_steps(seg[:, 0:2], W, H), to_steps(seg[:, 2:4], W, H)], 1).astype(np.int32)
        s0 = (0, 0) if start is None else tuple(int(v) for v in to_steps(np.asarray(start, np.float64).reshape(1, 2), W, H)[0])
        order, rev = order_fn(ends, np.zeros(len(seg), np.int32), 1, reverse=True, start=s0)
        seg = seg[np.asarray(order, np.int64)]
        seg = np.where(np.asarray(rev, bool)[:, None], seg[:, [2, 3, 0, 1]], seg)
    return np.ascontiguousarray(seg, np.int32), st


def fill_strokes(mask, w_src: int, h_src: int, cfg: Config, opts: dict, dev: Device | None = None, layer: int = 0, start=None, fill_fn=None, link_fn=None, order_fn=None):
    """the hatch of one layer as zigzags (include/orip.h: orip_fill_link) -> (polylines: a list of int32 [p, 2] in canvas pixels, in drawing order,
    {lib.FILL_STATS}, {lib.FILL_LINK_STATS}).  As fill_segments, which it mirrors: opts is an entry of fill_options that carries `reach`; link_fn stands in
    for Device.fill_link beside fill_fn / order_fn.  The link works on the segments as the device emitted them; order "nearest" then sends each stroke's
    first and last point through the same gcode_order_pens call, and a reversed stroke has its points reversed."""
    from .stream import to_steps
    if mask is not None and tuple(np.asarray(mask).shape) != (int(h_src), int(w_src)):
        raise ValueError(f"mask of shape {np.asarray(mask).shape} for a source of {w_src} x {h_src}")
    W, H = canvas_size_px(cfg)
    place = fill_placement(cfg, w_src, h_src)
    if fill_fn is None or link_fn is None:
        d = dev or device()
        fill_fn = fill_fn or (lambda *a: d.fill_mask(*a, layer=layer))
        link_fn = link_fn or (lambda *a: d.fill_link(*a, layer=layer))
    _, st = fill_fn(mask, W, H, place, opts["u"], opts["spacing"], opts["inset"], opts["min_len"], opts["flags"])
    off, pts, lst = link_fn(mask, place, opts["reach"])
    off, pts = np.asarray(off, np.int64).reshape(-1), np.asarray(pts, np.int32).reshape(-1, 2)
    strokes = [np.ascontiguousarray(pts[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    if opts["order"] == "nearest" and strokes:
        if order_fn is None:
            order_fn = (dev or device()).gcode_order_pens
        ends = np.concatenate([to_steps(pts[off[:-1]], W, H), to_steps(pts[off[1:] - 1], W, H)], 1).astype(np.int32)
        s0 = (0, 0) if start is None else tuple(int(v) for v in to_steps(np.asarray(start, np.float64).reshape(1, 2), W, H)[0])
        order, rev = order_fn(ends, np.zeros(len(strokes), np.int32), 1, reverse=True, start=s0)
        strokes = [np.ascontiguousarray(strokes[int(i)][::-1]) if r else strokes[int(i)] for i, r in zip(order, rev)]
    return strokes, st, lst


def fill_stroke_ops(strokes) -> List[dict]:
    """polylines as ops of stage 12's kind: {"type": "line", "points": float32 [p, 2]} in canvas pixels"""
    return [{"type": "line", "points": np.asarray(p, np.float32).reshape(-1, 2).copy()} for p in strokes]


def fill_ops(seg) -> List[dict]:
    """segments as ops of stage 12's kind: {"type": "line", "points": float32 [2, 2]} in canvas pixels"""
    return [{"type": "line", "points": np.asarray(s, np.float32).reshape(2, 2).copy()} for s in np.asarray(seg).reshape(-1, 4)]


def fill_stipple_radii(cfg: Config, opts: dict, w_src: int, h_src: int) -> Tuple[int, int]:
    """(clear_rad, tone_rad) of orip_fill_stipple in SOURCE pixels, from a stipple entry of fill_options and the placement num / den: clear_rad =
    ceil(inset den / num), tone_rad = floor(tone_radius den / num).  More than lib.FILL_STIPPLE_RAD_MAX is a ValueError naming inset_mm or tone_radius_mm;
    only a tone radius nobody stated (half the pitch) is capped there instead."""
    num, den, _, _ = fill_placement(cfg, w_src, h_src)
    clear_rad, tone_rad = -((-opts["inset"] * den) // num), (opts["tone_radius"] * den) // num
    if clear_rad > _l.FILL_STIPPLE_RAD_MAX:
        raise ValueError(f"fill: inset_mm is {opts['inset']} pixels, {clear_rad} pixels of the {w_src} x {h_src} image: at most {_l.FILL_STIPPLE_RAD_MAX}")
    if tone_rad > _l.FILL_STIPPLE_RAD_MAX:
        if opts["tone_radius_stated"]:
            raise ValueError(f"fill: tone_radius_mm is {opts['tone_radius']} pixels, {tone_rad} pixels of the {w_src} x {h_src} image: at most {_l.FILL_STIPPLE_RAD_MAX}")
        tone_rad = _l.FILL_STIPPLE_RAD_MAX
    return int(clear_rad), int(tone_rad)


def fill_dots(mask, tone, w_src: int, h_src: int, cfg: Config, opts: dict, dev: Device | None = None, layer: int = 0, start=None, stipple_fn=None, order_fn=None):
    """the dots of one layer (include/orip.h: orip_fill_stipple) -> (xy int32 [n, 2] in canvas pixels, in drawing order, {lib.FILL_STIPPLE_STATS}).  As
    fill_segments, which it mirrors: mask u8 [h_src, w_src] or None for the resident mask of `layer`; tone u8 [h_src, w_src], the grey source image, which is
    not passed on when the entry says tone = false; opts: a stipple entry of fill_options.  stipple_fn / order_fn stand in for Device.fill_stipple /
    Device.gcode_order_pens.  Order "nearest" sends every dot as the ends [x, y, x, y] of a stroke through gcode_order_pens: one group, nothing to reverse,
    from `start`."""
    from .stream import to_steps
    for what, a in (("mask", mask), ("tone", tone)):
        if a is not None and tuple(np.asarray(a).shape) != (int(h_src), int(w_src)):
            raise ValueError(f"{what} of shape {np.asarray(a).shape} for a source of {w_src} x {h_src}")
    W, H = canvas_size_px(cfg)
    clear_rad, tone_rad = fill_stipple_radii(cfg, opts, w_src, h_src)
    if stipple_fn is None:
        d = dev or device()
        stipple_fn = lambda *a: d.fill_stipple(*a, layer=layer)
    xy, st = stipple_fn(mask, tone if opts["tone"] else None, W, H, fill_placement(cfg, w_src, h_src), opts["lattice"], clear_rad, tone_rad, opts["lo"], opts["hi"], opts["flags"])
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    if opts["order"] == "nearest" and len(xy):
        if order_fn is None:
            order_fn = (dev or device()).gcode_order_pens
        p = to_steps(xy, W, H)
        s0 = (0, 0) if start is None else tuple(int(v) for v in to_steps(np.asarray(start, np.float64).reshape(1, 2), W, H)[0])
        order, _ = order_fn(np.concatenate([p, p], 1).astype(np.int32), np.zeros(len(xy), np.int32), 1, reverse=False, start=s0)
        xy = xy[np.asarray(order, np.int64)]
    return np.ascontiguousarray(xy, np.int32), st


def fill_dot_ops(xy) -> List[dict]:
    """dots as ops of stage 12's kind: {"type": "tap", "x": int, "y": int} in canvas pixels, what ops_from_device writes"""
    return [{"type": "tap", "x": int(x), "y": int(y)} for x, y in np.asarray(xy).reshape(-1, 2).tolist()]


def fill_layer(mask, w_src: int, h_src: int, cfg: Config, opts: dict, dev: Device | None = None, layer: int = 0, start=None) -> List[dict]:
    """the hatch of one layer as ops (fill_segments without the counts)"""
    seg, _ = fill_segments(mask, w_src, h_src, cfg, opts, dev, layer, start)
    return fill_ops(seg)


# ---------------------------------------------------------------- layer concurrency
_pool = None


def for_each_layer(fn, layers):
    """Run fn(layer) for every layer from its own host thread.  The per-layer entry points of liborip.so (05, 07, 08, 12)
    use one HIP stream and one scratch set per layer and ctypes drops the GIL during the call, so the latency-bound
    kernels of different layers overlap on the GPU (the reference loops over layers serially: 05:114, 07:99, 08:561, 12:200)."""
    global _pool
    layers = list(layers)
    if len(layers) <= 1 or os.environ.get("ORIP_SERIAL_LAYERS"):      # the switch is a profiling aid: kernels of one layer at a time
        return [fn(l) for l in layers]
    return list(_get_pool().map(fn, layers))


def _get_pool():
    global _pool
    if _pool is None:
        from concurrent.futures import ThreadPoolExecutor
        _pool = ThreadPoolExecutor(max_workers=_l.MAX_LAYERS + 2)
    return _pool


# ---------------------------------------------------------------- the resident end-to-end path
def run_path(bgr: np.ndarray, cfg: Config, dev: Device | None = None, centers: np.ndarray | None = None, upto: int = 12,
             fetch_ops: bool = True):
    """Stages 02 -> `upto` with every intermediate artefact resident on the GPU.  Device layer l carries the l-th darkest
    cluster, i.e. the name cluster_names(cfg)[l].  Returns {name: ops} (or None when upto < 12 / fetch_ops False)."""
    d = dev or device()
    names = list(cfg.color_names)
    K = max(2, len(names))
    lnames = cluster_names(cfg)[:K]
    H, W = bgr.shape[:2]
    d.set_image(bgr)
    if upto >= 5:
        d.contours_reserve(K)      # sizes stage 04's memo planes now; it clears nothing
    if centers is None:
        centers, _ = d.kmeans_fit_subsampled(SUBSAMPLE_LIMIT, K)
    d.extract_layers(np.asarray(centers, np.float32), want_counts=False)
    if upto < 3: return None
    _detect_edges_resident(d, cfg)
    if upto < 4: return None
    if upto < 5:
        d.find_contours()
        return None
    order = sorted(range(K), key=lambda l: (darkness_rank10(lnames[l]), names.index(lnames[l])))
    R = r_insert12(cfg)
    tail = None
    if upto >= 12:
        tail = (lambda l: ops_from_device(d, l, R)) if fetch_ops else (lambda l: d.plot_order(l, R))
    res = run_layer_pipelines(d, cfg, W, H, range(K), order if upto >= 10 else None, upto, tail)
    if upto < 12 or not fetch_ops:
        return None
    return {lnames[l]: res[l] for l in range(K)}


def run_layer_pipelines(d: Device, cfg: Config, W: int, H: int, layers, order, upto: int = 12, tail=None) -> dict:
    """Stages 04 -> 12 as one dependency-driven pipeline per layer (edges must be resident).  The reference runs stage after
    stage over all layers (pipeline.py:17-31); the only cross-layer dependency is stage 10, which visits the layers from dark
    to light and needs layer l's stage-08 output plus the raster painted by the layers before it (10:230-262).  So every
    layer walks 04 -> 05 -> 07 -> 08 on its own lane (host thread + HIP stream), the calling thread feeds the layers to
    stage 10 in `order` as they become ready, and `tail(layer)` (stage 12) runs as soon as the layer has left stage 10.
    order None: stop after stage min(upto, 8).  Returns {layer: tail result}."""
    layers = list(layers)
    d.contours_prepare()
    front = layer_front(d, cfg, W, H, upto)
    if order is None or os.environ.get("ORIP_SERIAL_LAYERS"):
        for_each_layer(front, layers)
        out = {}
        if order is not None:
            d.dedup_cross([l for l in order], params10(cfg))
            if tail is not None:
                out = dict(zip(layers, for_each_layer(tail, layers)))
        return out
    ready, errors = _start_fronts(front, layers, order)
    pool = _get_pool()
    d.dedup_cross_begin(params10(cfg))
    tails = {}
    for l in order:
        if l in ready:
            ready[l].wait()
        if errors:
            for e in ready.values(): e.wait()
            raise errors[0]
        d.dedup_cross_layer(l, defer_reorder=tail is not None and l in ready)      # the tail (stage 12) reorders on the layer's own lane
        if tail is not None and l in ready:
            tails[l] = pool.submit(tail, l)
    return {l: f.result() for l, f in tails.items()}


def _start_fronts(front, layers, order=None):
    """Submit front(layer) for every layer to the pool (layers that stage 10 visits first go first).  Returns
    ({layer: Event set when the layer is done or failed}, [exceptions])."""
    import threading
    pool = _get_pool()
    ready = {l: threading.Event() for l in layers}
    errors = []

    def guarded(l):
        try:
            front(l)
        except BaseException as e:      # surfaced on the calling thread
            errors.append(e)
        finally:
            ready[l].set()

    rank_of = (lambda l: order.index(l) if l in order else len(order)) if order else (lambda l: 0)
    for l in sorted(layers, key=rank_of):
        pool.submit(guarded, l)
    return ready, errors


def layer_front(d: Device, cfg: Config, W: int, H: int, upto: int = 8):
    """front(layer): stages 04 (walks of the layer) -> 05 -> 07 -> 08 on the layer's lane; needs d.contours_prepare() first."""
    sx, sy, dx, dy = scale_factors(cfg, W, H)
    p8 = params08(cfg)

    def front(l):
        d.layer_front(l, sx, sy, dx, dy, 8 if upto >= 8 else (7 if upto >= 7 else 5), p8)
    return front
