#!/usr/bin/env python3
"""tests/golden/make_golden_stream_preview.py -- golden vectors for the stream preview (14_preview_stream.py over
shared/omnirevolve_plotter_stream_previewer.py).

Runs ONLY in the build container (needs /root/reference).  pygame is not installed there: a small recording stub is registered as `pygame`
(the previewer only needs init, a font, display.Info / set_mode, Surface fill / clip, Rect and draw.line / draw.circle).  Its display reports a
screen large enough that the render surface gets the requested size, as the headless mode of the previewer has it.  Then the previewer's own
StreamDecoder and PlotterPreview._replay_to(len(commands)) run on every stream; what is recorded, as arrays only:
  * <run>_stats     int64 [17]: the previewer's Statistics in field order, then unknown_service_bytes (its stderr warnings) and commands
  * <run>_lines     int32 [n, 7]: every draw.line call (x1, y1, x2, y2, r, g, b); <run>_line_clip int32 [n, 4] the active clip (-1: none)
  * <run>_circles   int32 [m, 6]: every draw.circle call (cx, cy, radius, r, g, b); <run>_circ_clip the same
  * <run>_surface (w, h), <run>_ws (workspace rect), <run>_scale (step_scale), <run>_cfg (W, H, invert_y, clip, background_white, render_taps,
    render width / height requested), <run>_palette uint8 [4, 3], <run>_stream: the stream's key (golden_stream.npz key or synth_* here)
pygame's scan conversion is NOT pinned: the tests derive pixels from the logged calls only where the previewer's geometry makes that
exact (step_scale <= 1: every line joins two pixels at most one apart).   Usage: python tests/golden/make_golden_stream_preview.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHARED = "/root/reference/shared"


class Rect:
    def __init__(self, x, y, w, h):
        self.x, self.y, self.w, self.h = int(x), int(y), int(w), int(h)
        self.width, self.height = self.w, self.h

    def tuple(self):
        return (self.x, self.y, self.w, self.h)


class Surface:
    def __init__(self, size):
        self.size = tuple(size)
        self.clip = None

    def fill(self, c):
        pass

    def get_clip(self):
        return self.clip

    def set_clip(self, r):
        self.clip = r

    def get_size(self):
        return self.size


LOG = {"lines": [], "line_clip": [], "circles": [], "circ_clip": []}


def _clip_of(s):
    return list(s.clip.tuple()) if s.clip is not None else [-1, -1, -1, -1]


def _line(surf, color, p1, p2, width=1):
    assert width == 1
    LOG["lines"].append([int(p1[0]), int(p1[1]), int(p2[0]), int(p2[1]), *[int(v) for v in color]]); LOG["line_clip"].append(_clip_of(surf))


def _circle(surf, color, center, radius, width=0):
    assert width == 0
    LOG["circles"].append([int(center[0]), int(center[1]), int(radius), *[int(v) for v in color]]); LOG["circ_clip"].append(_clip_of(surf))


def make_pygame_stub():
    pg = types.ModuleType("pygame")
    pg.RESIZABLE = 16
    pg.init = lambda: None
    pg.quit = lambda: None
    pg.Rect = Rect
    pg.Surface = Surface
    pg.font = types.SimpleNamespace(Font=lambda *a, **k: object())
    pg.display = types.SimpleNamespace(Info=lambda: types.SimpleNamespace(current_w=100000, current_h=100000),
                                       set_mode=lambda size, flags=0: Surface(size), set_caption=lambda *a: None)
    pg.time = types.SimpleNamespace(Clock=lambda: object())
    pg.draw = types.SimpleNamespace(line=_line, circle=_circle)
    return pg


sys.modules["pygame"] = make_pygame_stub()
sys.path.insert(0, SHARED)
import omnirevolve_plotter_stream_previewer as PV  # noqa: E402


def synth_stream(seed: int, n_runs: int, eof: str) -> bytes:
    """every byte class: pen up / down / tap, colours 0..7, speeds, unknown service bytes, single and double steps in straight runs that start near
    the centre of a 600 x 450 canvas, leave it on every side and turn back towards the centre; eof = 'mid' (EOF, then a tail), 'none' (no EOF at
    all), 'end'"""
    rng = np.random.default_rng(seed)
    DXY = [(0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1)]
    out = bytearray([0xC0 | (1 << 3) | 1] * 110 + [0x80 | (2 << 3)] * 80)     # pen up to (300, 220)
    x, y = 300, 220
    unknown = [0x00, 0x04, 0x05, 0x06, 0x07, 0x10, 0x20, 0x30, 0x3E]
    for r in range(n_runs):
        u = rng.random()
        if u < 0.15:
            out.append(int(rng.choice([0x01, 0x02, 0x02, 0x02, 0x03])))
        elif u < 0.25:
            out.append(0x08 + int(rng.integers(0, 8)))
        elif u < 0.30:
            out.append(0x40 | int(rng.integers(0, 64)))
        elif u < 0.33:
            out.append(int(rng.choice(unknown)))
        else:
            if rng.random() < 0.5:                       # back towards the centre
                heading = min(range(8), key=lambda h: (x + 50 * DXY[h][0] - 300) ** 2 + (y + 50 * DXY[h][1] - 225) ** 2)
            else:
                heading = int(rng.integers(0, 8))
            L = int(rng.integers(1, 120)) if rng.random() < 0.8 else int(rng.integers(200, 500))
            for _ in range(L):
                h2 = (heading + int(rng.integers(-1, 2))) & 7 if rng.random() < 0.1 else heading
                if rng.random() < 0.5:
                    out.append(0x80 | (heading << 3)); x += DXY[heading][0]; y += DXY[heading][1]
                else:
                    out.append(0xC0 | (heading << 3) | h2); x += DXY[heading][0] + DXY[h2][0]; y += DXY[heading][1] + DXY[h2][1]
        if eof == "mid" and r == n_runs // 2:
            out.append(0x3F)
    if eof == "end":
        out.append(0x3F)
    return bytes(out)


def record(data: bytes, W, H, invert_y, clip, bg_white, taps, rw, rh, palette):
    for k in LOG:
        LOG[k].clear()
    cfg = PV.Config(render_width_px=rw, render_height_px=rh, canvas_steps_w=W, canvas_steps_h=H, invert_y=bool(invert_y), render_taps=bool(taps),
                    colors=tuple(tuple(c) for c in palette), background_white=bool(bg_white), clip_to_canvas=bool(clip))
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        dec = PV.StreamDecoder(data)
    with contextlib.redirect_stdout(io.StringIO()):
        sim = PV.PlotterPreview(dec, cfg)
        sim._replay_to(len(dec.commands))
    s = sim.stats
    unknown = sum(1 for line in err.getvalue().splitlines() if line.startswith("WARNING: Unknown service byte"))
    stats = [s.total_bytes, s.service_bytes, s.step_bytes, s.single_steps, s.double_steps, s.steps_total, s.pen_down_segments, s.taps,
             s.color_changes, s.speed_changes, int(s.eof_seen), s.tail_after_eof, s.off_canvas_draws, s.final_x, s.final_y, unknown, len(dec.commands)]
    r = {"stats": np.array(stats, np.int64),
         "lines": np.array(LOG["lines"], np.int32).reshape(-1, 7), "line_clip": np.array(LOG["line_clip"], np.int32).reshape(-1, 4),
         "circles": np.array(LOG["circles"], np.int32).reshape(-1, 6), "circ_clip": np.array(LOG["circ_clip"], np.int32).reshape(-1, 4),
         "surface": np.array([sim.render_w, sim.render_h], np.int32), "ws": np.array(sim.ws_rect.tuple(), np.int32),
         "scale": np.array(sim.step_scale, np.float64),
         "cfg": np.array([W, H, int(invert_y), int(clip), int(bg_white), int(taps), rw, rh], np.int64), "palette": np.array(palette, np.uint8)}
    return r


RGBK = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0))
CMYW = ((0, 255, 255), (255, 0, 255), (255, 255, 0), (255, 255, 255))


def main():
    GS = np.load(os.path.join(HERE, "golden_stream.npz"))
    streams = {"e2e_a_bin": bytes(GS["e2e_a_bin"]), "e2e_b_bin": bytes(GS["e2e_b_bin"]), "e2e_b_remap_bin": bytes(GS["e2e_b_remap_bin"])}
    g = {}
    synth = {"synth_mid": synth_stream(1, 120, "mid"), "synth_none": synth_stream(2, 120, "none"), "synth_end": synth_stream(7, 60, "end")}
    for k, v in synth.items():
        g[k] = np.frombuffer(v, np.uint8)
    streams.update(synth)
    # (run, stream, W, H, invert_y, clip, background_white, render_taps, render w, h, palette)
    runs = [("a_stage", "e2e_a_bin", 8400, 11880, 1, 1, 1, 1, 1200, 900, RGBK),          # the reference stage's parameters
            ("b_stage", "e2e_b_bin", 8400, 11880, 1, 1, 1, 1, 1200, 900, RGBK),
            ("b_remap", "e2e_b_remap_bin", 8400, 11880, 1, 1, 1, 1, 1200, 900, CMYW),   # colours 4..7 from the remap
            ("a_canvas", "e2e_a_bin", 1000, 1200, 0, 1, 0, 1, 1000, 1200, RGBK)]        # render = canvas (scale 1), no inversion, black
    for s in synth:
        runs += [(f"{s}_base", s, 600, 450, 1, 1, 1, 1, 500, 400, RGBK),
                 (f"{s}_inv0", s, 600, 450, 0, 1, 1, 1, 500, 400, RGBK),
                 (f"{s}_noclip", s, 600, 450, 1, 0, 1, 1, 500, 400, RGBK),
                 (f"{s}_black_notaps", s, 600, 450, 1, 1, 0, 0, 500, 400, CMYW),
                 (f"{s}_small", s, 600, 450, 0, 1, 1, 1, 120, 90, RGBK),               # below 400 x 300: clamped
                 (f"{s}_unit", s, 600, 450, 1, 1, 1, 1, 600, 450, RGBK),               # render = canvas: step_scale 1
                 (f"{s}_big", s, 150, 120, 1, 0, 1, 1, 600, 480, RGBK)]                # step_scale 4: draw calls pinned, pixels not
    names = []
    for name, s, W, H, inv, clip, bg, taps, rw, rh, pal in runs:
        r = record(streams[s], W, H, inv, clip, bg, taps, rw, rh, pal)
        for k, v in r.items():
            g[f"{name}_{k}"] = v
        g[f"{name}_stream"] = np.array(s)
        names.append(name)
        print(f"{name:22s} {len(streams[s]):6d} B  cmds {int(r['stats'][16]):6d}  lines {len(r['lines']):6d}  circles {len(r['circles']):4d}  "
              f"surface {tuple(r['surface'])}  ws {tuple(r['ws'])}  scale {float(r['scale']):.4f}")
    g["runs"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "golden_stream_preview.npz"), **g)
    print("golden_stream_preview.npz:", len(g), "arrays,", os.path.getsize(os.path.join(HERE, "golden_stream_preview.npz")), "bytes")


if __name__ == "__main__":
    main()
