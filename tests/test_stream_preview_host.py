"""Stage 14 (stream preview) on the CPU: the numpy double of the GPU path (tests/stream_preview_double.py) against the reference previewer's own
statistics and draw-call log (tests/golden/golden_stream_preview.npz), and the host rules of orip/stream_preview.py against the reference stage's."""
import json
import os
import sys

import numpy as np
import pytest

from util import load
import stream_preview_double as D

G = load("golden_stream_preview.npz")
GS = load("golden_stream.npz")
RUNS = [str(r) for r in G["runs"]]


def _sp():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omnirevolve-image-processor_amd"))
    from orip import stream_preview as SP
    return SP


def stream_of(run):
    key = str(G[f"{run}_stream"])
    return bytes(G[key]) if key in G.files else bytes(GS[key])


def args_of(run):
    """(data, W, H, rw, rh, invert_y, clip, render_taps, background_white, palette) with the headless render clamp applied"""
    W, H, inv, clip, bg, taps, rw, rh = (int(v) for v in G[f"{run}_cfg"])
    rw, rh = _sp().render_size(rw, rh)
    return stream_of(run), W, H, rw, rh, bool(inv), bool(clip), bool(taps), bool(bg), [tuple(int(c) for c in p) for p in G[f"{run}_palette"]]


def golden_rgb_from_calls(run, rw, rh, bg_white):
    """the pixels the logged line calls set when every line joins pixels at most one apart (step_scale <= 1): its two ends, inside the clip;
    mask = pixels no logged disc can reach (pygame's disc is not pinned)"""
    img = np.full((rh, rw, 3), 255 if bg_white else 0, np.uint8)
    L, LC = G[f"{run}_lines"].astype(np.int64), G[f"{run}_line_clip"].astype(np.int64)
    assert np.all(np.abs(L[:, 2] - L[:, 0]) <= 1) and np.all(np.abs(L[:, 3] - L[:, 1]) <= 1)
    for (x1, y1, x2, y2, r, g, b), (cx, cy, cw, ch) in zip(L.tolist(), LC.tolist()):
        X0, Y0, X1, Y1 = (0, 0, rw, rh) if cw < 0 else (max(cx, 0), max(cy, 0), min(cx + cw, rw), min(cy + ch, rh))
        for px, py in ((x1, y1), (x2, y2)):
            if X0 <= px < X1 and Y0 <= py < Y1:
                img[py, px] = (r, g, b)
    mask = np.ones((rh, rw), bool)
    for cx, cy, rad, *_ in G[f"{run}_circles"].tolist():
        mask[max(0, cy - rad - 1):max(0, cy + rad + 2), max(0, cx - rad - 1):max(0, cx + rad + 2)] = False
    return img, mask


@pytest.mark.parametrize("run", RUNS)
def test_double_statistics_match_reference(run):
    data, W, H, rw, rh, inv, clip, taps, bg, pal = args_of(run)
    st, _ = D.replay(data, W, H, rw, rh, inv, clip, taps, pal)
    assert [st[k] for k in D.FIELDS] == G[f"{run}_stats"].tolist()


@pytest.mark.parametrize("run", RUNS)
def test_double_draw_calls_match_reference(run):
    """every draw.line / draw.circle call of the previewer: end points, colour, radius and the clip active at the call"""
    data, W, H, rw, rh, inv, clip, taps, bg, pal = args_of(run)
    assert (rw, rh) == tuple(G[f"{run}_surface"].tolist())
    scale, ox, oy, uw, uh = D.geometry(W, H, rw, rh)
    assert scale == float(G[f"{run}_scale"]) and (ox, oy, uw, uh) == tuple(G[f"{run}_ws"].tolist())
    _, calls = D.replay(data, W, H, rw, rh, inv, clip, taps, pal)
    P = np.asarray(pal, np.int64)
    gl, gc = G[f"{run}_lines"].astype(np.int64), G[f"{run}_circles"].astype(np.int64)
    assert np.array_equal(calls["lines"], gl[:, :4]) and np.array_equal(P[calls["line_col"]].reshape(-1, 3), gl[:, 4:])
    assert np.array_equal(calls["circles"], gc[:, :3]) and np.array_equal(P[calls["circ_col"]].reshape(-1, 3), gc[:, 3:])
    want_clip = list(calls["clip"]) if calls["clip"] is not None else [-1, -1, -1, -1]
    for k in ("line_clip", "circ_clip"):
        assert all(c == want_clip for c in G[f"{run}_{k}"].tolist())


@pytest.mark.parametrize("run", [r for r in RUNS if float(G[f"{r}_scale"]) <= 1.0])
def test_double_pixels_match_reference_calls(run):
    data, W, H, rw, rh, inv, clip, taps, bg, pal = args_of(run)
    rgb, _ = D.preview(data, W, H, rw, rh, inv, clip, taps, bg, pal)
    want, mask = golden_rgb_from_calls(run, rw, rh, bg)
    assert rgb.shape == (rh, rw, 3)
    assert np.array_equal(rgb[mask], want[mask])
    if len(G[f"{run}_lines"]):
        assert (rgb[mask] != (255 if bg else 0)).any()


def test_double_disc_and_dda_stand_ins():
    si, sj = D.disc_offsets(5)
    assert len(si) == 81 and (si * si + sj * sj <= 25).all()
    seg, px, py = D.line_pixels([[0, 0, 4, 2], [3, 3, 3, 3], [5, 5, 6, 4]])
    assert seg.tolist() == [0] * 5 + [1] + [2, 2]
    assert list(zip(px.tolist(), py.tolist())) == [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2), (3, 3), (5, 5), (6, 4)]


def test_parse_color_rules():
    SP = _sp()
    assert SP.parse_color("R") == (255, 0, 0) and SP.parse_color(" magenta ") == (255, 0, 255) and SP.parse_color("k") == (0, 0, 0)
    assert SP.parse_color("#0a10FF") == (10, 16, 255)
    assert SP.parse_color("300,-4,17") == (255, 0, 17)
    for bad in ("purple", "#12345", "1,2"):
        with pytest.raises(ValueError):
            SP.parse_color(bad)


def test_render_size_clamp_and_geometry():
    SP = _sp()
    assert SP.render_size(1200, 900) == (1200, 900) and SP.render_size(120, 90) == (400, 300) and SP.render_size(399, 5000) == (400, 5000)
    assert SP.tap_radius() == 5
    for run in RUNS:
        W, H, *_ , rw, rh = (int(v) for v in G[f"{run}_cfg"])
        rw, rh = SP.render_size(rw, rh)
        g = SP.geometry(W, H, rw, rh)
        assert g["step_scale"] == float(G[f"{run}_scale"])
        assert (g["offset_x"], g["offset_y"], g["used_w"], g["used_h"]) == tuple(G[f"{run}_ws"].tolist())


def test_canvas_resolution(tmp_path):
    """stream_meta.json wins; else target_*_mm at 40 steps per mm, whatever pixels_per_mm says (steps_per_mm is not a Config field)"""
    SP = _sp()
    from orip.config import Config
    cfg = Config(); cfg.pixels_per_mm = 6; cfg.target_width_mm = 100; cfg.target_height_mm = 50
    assert SP.canvas_for_output(str(tmp_path), cfg) == (4000, 2000, 1)
    assert SP.canvas_for_output(str(tmp_path), Config()) == (8400, 11880, 1)
    (tmp_path / "stream_meta.json").write_text(json.dumps({"canvas_steps": [1234, 567], "invert_y": False}))
    assert SP.canvas_for_output(str(tmp_path), cfg) == (1234, 567, 0)
    (tmp_path / "stream_meta.json").write_text(json.dumps({}))
    assert SP.canvas_for_output(str(tmp_path), cfg) == (8400, 11880, 1)


def test_print_stats_format():
    import io
    SP = _sp()
    st = dict(zip(D.FIELDS, G["a_stage_stats"].tolist()))
    buf = io.StringIO()
    SP.print_stats(st, file=buf)
    lines = buf.getvalue().splitlines()
    assert lines[1] == "=== Statistics ===" and lines[2] == f"Total bytes: {st['total_bytes']:,}".replace(",", " ")
    assert lines[-2].startswith("EOF seen: True  Tail after EOF: ") and lines[-1] == f"Final position: ({st['final_x']}, {st['final_y']})"
