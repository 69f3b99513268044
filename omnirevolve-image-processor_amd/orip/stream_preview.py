"""Headless preview of a plotter stream (the reference's 14_preview_stream.py over shared/omnirevolve_plotter_stream_previewer.py, `-o out.png`):
decode plot_stream.bin, replay it and draw what the pen would draw.  The decode, the replay and the raster run on the GPU
(include/orip.h: orip_stream_preview, csrc/stream_preview.hip); this module holds the host rules around them:

  * parse_color           the previewer's colour specs (named, #rrggbb, "r,g,b" clamped to 0..255)
  * render_size           the headless render surface: (max(400, w), max(300, h)) -- the previewer's
                          max(400, min(w, window - margins)) with a window large enough for the request
  * geometry              step_scale / workspace rect in IEEE double, in the previewer's order of operations
  * canvas_for_output     canvas size in steps and Y inversion as the reference stage resolves them: stream_meta.json (canvas_steps,
                          invert_y) when present, else target_*_mm * steps_per_mm.  steps_per_mm is NOT a Config field, so the
                          stage's getattr default of 40 always applies, whatever pixels_per_mm says -- kept as the reference has it
  * print_stats / main    the statistics block of the previewer's _print_stats and its headless command line

Statistics come back as a dict in STAT_FIELDS order: the previewer's Statistics, then unknown_service_bytes and commands."""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

STAT_FIELDS = ("total_bytes", "service_bytes", "step_bytes", "single_steps", "double_steps", "steps_total", "pen_down_segments", "taps",
               "color_changes", "speed_changes", "eof_seen", "tail_after_eof", "off_canvas_draws", "final_x", "final_y",
               "unknown_service_bytes", "commands")
# flags of orip_stream_preview
FLAG_INVERT_Y, FLAG_CLIP, FLAG_TAPS, FLAG_BG_WHITE = 1, 2, 4, 8
PEN_DIAM_PX = 10                       # the previewer's tap diameter, the same for every palette index
DEFAULT_PALETTE = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0))   # R, G, B, K
STEPS_PER_MM = 40                      # the reference stage's getattr(cfg, "steps_per_mm", 40): never a Config field


def parse_color(spec: str) -> Tuple[int, int, int]:
    s = spec.strip().lower()
    named = {"r": (255, 0, 0), "red": (255, 0, 0), "g": (0, 255, 0), "green": (0, 255, 0), "b": (0, 0, 255), "blue": (0, 0, 255),
             "k": (0, 0, 0), "black": (0, 0, 0), "w": (255, 255, 255), "white": (255, 255, 255), "y": (255, 255, 0), "yellow": (255, 255, 0),
             "c": (0, 255, 255), "cyan": (0, 255, 255), "m": (255, 0, 255), "magenta": (255, 0, 255)}
    if s in named:
        return named[s]
    if s.startswith("#") and len(s) == 7:
        return int(s[1:3], 16), int(s[3:5], 16), int(s[5:7], 16)
    if "," in s:
        r, g, b = (int(p) for p in s.split(","))
        return max(0, min(255, r)), max(0, min(255, g)), max(0, min(255, b))
    raise ValueError(f"Bad color spec: {spec}")


def render_size(width: int, height: int) -> Tuple[int, int]:
    return max(400, int(width)), max(300, int(height))


def tap_radius(diam_px: int = PEN_DIAM_PX) -> int:
    return max(1, int(diam_px) // 2)


def geometry(W: int, H: int, rw: int, rh: int) -> Dict[str, float]:
    """_rebuild_render_surface: uniform scale, workspace rect (offset_x, offset_y, used_w, used_h) inside the rw x rh surface"""
    scale = min(rw / max(1, W), rh / max(1, H))
    used_w, used_h = int(W * scale), int(H * scale)
    return {"step_scale": scale, "offset_x": (rw - used_w) // 2, "offset_y": (rh - used_h) // 2, "used_w": used_w, "used_h": used_h}


def canvas_for_output(output_dir: str, cfg) -> Tuple[int, int, int]:
    """(W, H, invert_y) of the reference stage 14: stream_meta.json first, else the target size in mm at 40 steps per mm"""
    meta_path = os.path.join(output_dir, "stream_meta.json")
    if os.path.exists(meta_path):
        with open(meta_path, "r", encoding="utf-8") as f:
            meta = json.load(f)
        W, H = meta.get("canvas_steps", [8400, 11880])
        return int(W), int(H), 1 if meta.get("invert_y", True) else 0
    spm = getattr(cfg, "steps_per_mm", STEPS_PER_MM)
    return int(getattr(cfg, "target_width_mm", 210) * spm), int(getattr(cfg, "target_height_mm", 297) * spm), 1


def flags_of(invert_y: bool, clip: bool, render_taps: bool, background_white: bool) -> int:
    return (FLAG_INVERT_Y if invert_y else 0) | (FLAG_CLIP if clip else 0) | (FLAG_TAPS if render_taps else 0) | (FLAG_BG_WHITE if background_white else 0)


def preview(dev, data: bytes, W: int, H: int, render_w: int = 1200, render_h: int = 900, invert_y: bool = True, clip: bool = True,
            render_taps: bool = True, background_white: bool = True, palette: Sequence[Tuple[int, int, int]] = DEFAULT_PALETTE):
    """decode + draw on the device: (rgb uint8 [rh, rw, 3], stats dict); the render request goes through the headless clamp"""
    rw, rh = render_size(render_w, render_h)
    return dev.stream_preview(np.frombuffer(bytes(data), np.uint8), W, H, rw, rh, flags_of(invert_y, clip, render_taps, background_white),
                              palette, tap_radius())


def save_png(rgb: np.ndarray, path: str) -> None:
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(rgb, np.uint8), "RGB").save(path)


def _F(x) -> str:
    return f"{int(x):,}".replace(",", " ")


def print_stats(st: Dict[str, int], file=None) -> None:
    """the previewer's _print_stats block, on stderr by default"""
    out = file or sys.stderr
    print("\n=== Statistics ===", file=out)
    print(f"Total bytes: {_F(st['total_bytes'])}", file=out)
    print(f"Step bytes: {_F(st['step_bytes'])}  Service bytes: {_F(st['service_bytes'])}", file=out)
    print(f"Steps: {_F(st['steps_total'])}  Singles: {_F(st['single_steps'])}  Doubles: {_F(st['double_steps'])}", file=out)
    print(f"PenDown segments: {_F(st['pen_down_segments'])}  Taps: {_F(st['taps'])}", file=out)
    print(f"Color changes: {_F(st['color_changes'])}  Speed changes: {_F(st['speed_changes'])}", file=out)
    print(f"Off-canvas draws: {_F(st['off_canvas_draws'])}", file=out)
    print(f"EOF seen: {bool(st['eof_seen'])}  Tail after EOF: {_F(st['tail_after_eof'])}", file=out)
    print(f"Final position: ({st['final_x']}, {st['final_y']})", file=out)


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(description="Headless plotter stream preview on the GPU (step/service stream -> PNG)")
    ap.add_argument("input", help="Input binary stream file")
    ap.add_argument("-o", "--output", required=True, help="Save rendered PNG to file")
    ap.add_argument("--render-width", type=int, default=1200)
    ap.add_argument("--render-height", type=int, default=900)
    ap.add_argument("--canvas-w-steps", type=int, default=13210)
    ap.add_argument("--canvas-h-steps", type=int, default=13019)
    ap.add_argument("--invert-y", type=int, choices=[0, 1], default=1)
    ap.add_argument("--background-white", type=int, choices=[0, 1], default=1)
    ap.add_argument("--render-taps", type=int, choices=[0, 1], default=1)
    ap.add_argument("--no-clip", action="store_true", help="Do not clip drawing to canvas")
    ap.add_argument("--stats-json", default=None, help="also write the statistics as JSON")
    for i, d in enumerate("RGBK"):
        ap.add_argument(f"--c{i}", default=d)
    a = ap.parse_args(argv)
    palette = tuple(parse_color(getattr(a, f"c{i}")) for i in range(4))
    with open(a.input, "rb") as f:
        data = f.read()
    from orip.device import Device
    dev = Device(0)
    try:
        rgb, st = preview(dev, data, a.canvas_w_steps, a.canvas_h_steps, a.render_width, a.render_height, bool(a.invert_y), not a.no_clip,
                          bool(a.render_taps), bool(a.background_white), palette)
    finally:
        dev.close()
    rw, rh = render_size(a.render_width, a.render_height)
    print(f"Canvas steps: {a.canvas_w_steps}x{a.canvas_h_steps}")
    print(f"Render surface: {rw}x{rh} px")
    save_png(rgb, a.output)
    print(f"Image saved: {a.output}")
    if a.stats_json:
        with open(a.stats_json, "w", encoding="utf-8") as f:
            json.dump(st, f, indent=2)
    print_stats(st)
    return 0


if __name__ == "__main__":
    sys.exit(main())
