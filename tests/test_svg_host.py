"""svg2stream on the CPU: the parser against hand-computed segment tables, the tokenizer on the compact forms, fit_transform against recorded parameters, the
numpy double of the fit against the reference's scale_and_offset_gcode bit for bit (every recorded value), the chord contract for every curve of every
fixture, host arcs against their true ellipses, the whole host path with the doubles of tests/svg_double.py injected against the streams the reference's
gcode2stream wrote, and the G-code text.  Fixture: tests/golden/golden_svg.npz (make_golden_svg.py).  No recorded case is left out."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from util import load
import svg_double as SD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = load("golden_svg.npz")
ARGS = json.loads(bytes(G["run_args"]).decode())
RUNS = json.loads(bytes(G["run_cases"]).decode())
NAMES = json.loads(bytes(G["svg_names"]).decode())
FIT_COUNT = int(G["fit_count"][0])
K = 4.0 / 3.0 * math.tan(math.pi / 8.0)


def svg_text(name):
    return bytes(G[f"svg_{name}"]).decode()


def options_for(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def table_of(name):
    from orip.svg import parse_svg
    return parse_svg(svg_text(name))


def kinds(t):
    return "".join(" LQC"[k] for k in t.kind)


# ------------------------------------------------------------------ parser
# per fixture: kinds of all segments, subpath ranges, closed flags, number of matrices, canvas height -- worked out by hand from the SVG texts
STRUCTURE = {
    "elements": ("LLL" "L" "LLL" "LLL" "LLLL" "LCLCLCLC" "CCCC" "CCCC" "CCCC" "L", [0, 3, 4, 7, 10, 14, 22, 26, 30, 34, 35], [1, 0, 0, 1, 1, 1, 1, 1, 1, 0], 1, 150.0),
    "transforms": ("LLLL" "Q" "CCCC" "CCCC" "LL", [0, 4, 5, 9, 13, 15], [1, 0, 1, 1, 0], 8, 300.0),
    "commands_abs": ("LLLCCQQCCL" "QCL", [0, 10, 13], [1, 0], 1, 120.0),
    "commands_rel": ("LLLCCQQCCL" "QCL", [0, 10, 13], [1, 0], 1, 120.0),
    "compact": ("LLLLL" "CCQQCCC" "LLLL", [0, 5, 12, 16], [1, 0, 0], 1, 50.0),
    "arcs": ("CC" "CC" "CCC" "CCC" "CCC" "CC" "CC" "LL" "CCCC", [0, 2, 4, 7, 10, 15, 17, 19, 23], [0] * 8, 1, 300.0),      # the rotated large arc turns by 180..270 degrees
    "malformed": ("LL" "L" "L", [0, 2, 3, 4], [0, 0, 0], 1, 100.0),
    "zero_area": ("L" "L", [0, 1, 2], [0, 0], 1, 100.0),
    "empty": ("", [0], [], 1, 100.0),
    "viewbox_only": ("C" "LCLCLCLC", [0, 1, 9], [0, 1], 1, 49.0),
    "loop": ("C", [0, 1], [0], 1, 10.0),
    "loop_flat": ("C", [0, 1], [0], 1, 10.0),
}


def test_every_fixture_has_a_hand_table():
    assert sorted(STRUCTURE) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_parser_structure(name):
    t = table_of(name)
    want_kinds, sub_off, closed, n_mats, height = STRUCTURE[name]
    assert kinds(t) == want_kinds and t.sub_off.tolist() == sub_off
    assert t.closed.tolist() == closed and len(t.mats) == n_mats and t.canvas_height == height
    assert t.kind.dtype == np.int32 and t.ctrl.shape == (t.n_seg, 4, 2) and t.ctrl.dtype == np.float64 and t.mat.dtype == np.int32 and t.sub_off.dtype == np.int64
    # every segment starts where its predecessor in the subpath ends
    end = t.ctrl[np.arange(t.n_seg), np.where(t.kind <= 1, 1, t.kind)] if t.n_seg else np.zeros((0, 2))
    inner = np.ones(t.n_seg, bool); inner[t.sub_off[:-1]] = False
    assert np.array_equal(t.ctrl[inner, 0], end[np.nonzero(inner)[0] - 1])
    for p in range(t.n_sub):
        if t.closed[p]:
            assert np.array_equal(end[t.sub_off[p + 1] - 1], t.ctrl[t.sub_off[p], 0])


def seg(t, s):
    return t.ctrl[s, :max(2, int(t.kind[s]) + 1) if t.kind[s] > 1 else 2].tolist()


def test_parser_elements_by_hand():
    t = table_of("elements")
    assert [seg(t, s) for s in range(3)] == [[[10, 10], [60, 10]], [[60, 10], [60, 40]], [[60, 40], [10, 10]]]                  # path, closed by z
    assert seg(t, 3) == [[5, 140], [195, 145]]                                                                                  # line
    assert [seg(t, s)[1] for s in range(4, 7)] == [[80, 30], [90, 10], [100, 30]]                                               # polyline
    assert [seg(t, s) for s in range(7, 10)] == [[[110, 10], [130, 10]], [[130, 10], [120, 35]], [[120, 35], [110, 10]]]        # polygon
    assert [seg(t, s)[1] for s in range(10, 14)] == [[50, 50], [50, 80], [10, 80], [10, 50]] and seg(t, 10)[0] == [10, 50]      # rect
    # rounded rect 60,50 40x30 rx 8 ry 5: top edge, then the top right corner from (92, 50) round (100, 50) to (100, 55)
    assert seg(t, 14) == [[68, 50], [92, 50]]
    assert seg(t, 15) == [[92, 50], [92 + K * 8, 50], [100, 55 + K * (50 - 55)], [100, 55]]
    assert seg(t, 16) == [[100, 55], [100, 75]] and seg(t, 21)[3] == [68, 50]
    # rx = 15 alone on a 30 x 30 rect: ry follows, the straight edges vanish
    assert seg(t, 22)[0] == [125, 50] and seg(t, 22)[3] == [140, 65] and seg(t, 25)[3] == [125, 50]
    # circle 160,30 r 20: from (180, 30) round (180, 50) to (160, 50)
    assert seg(t, 26) == [[180, 30], [180, 30 + K * 20], [160 + K * 20, 50], [160, 50]]
    assert [seg(t, s)[3] for s in range(26, 30)] == [[160, 50], [140, 30], [160, 10], [180, 30]]
    assert [seg(t, s)[3] for s in range(30, 34)] == [[160, 115], [130, 100], [160, 85], [190, 100]]                             # ellipse
    assert seg(t, 34) == [[10, 100], [100, 130]]                                                                                # the nested line; nothing of defs, clipPath, ... , display none
    assert t.ctrl.max() < 200


def test_parser_commands_by_hand():
    t = table_of("commands_abs")
    assert [seg(t, s) for s in range(3)] == [[[10, 10], [30, 10]], [[30, 10], [50, 10]], [[50, 10], [50, 30]]]
    assert seg(t, 3) == [[50, 30], [60, 40], [70, 40], [80, 30]]
    assert seg(t, 4) == [[80, 30], [90, 20], [100, 20], [110, 30]]                   # S: the handle (70, 40) reflected in (80, 30)
    assert seg(t, 5) == [[110, 30], [100, 50], [90, 40]]
    assert seg(t, 6) == [[90, 40], [80, 30], [70, 50]]                               # T: the handle (100, 50) reflected in (90, 40)
    assert seg(t, 7)[0] == [70, 50] and seg(t, 8)[3] == [40, 50]                     # the arc: half an ellipse in two pieces
    assert seg(t, 9) == [[40, 50], [10, 10]]                                         # Z
    assert seg(t, 10) == [[10, 70], [10, 70], [30, 70]]                              # T after M: the handle is the current point
    assert seg(t, 11) == [[30, 70], [30, 70], [40, 90], [50, 70]]                    # S after T: likewise
    assert seg(t, 12) == [[50, 70], [10, 110]]
    r = table_of("commands_rel")                                                     # the same drawing in relative commands
    assert np.array_equal(r.kind, t.kind) and np.array_equal(r.ctrl, t.ctrl) and np.array_equal(r.sub_off, t.sub_off)


def test_parser_small_fixtures_by_hand():
    t = table_of("compact")                                                          # M1.5.5-1-2 1e-3,4l3-3 2 2z m5,5 ...
    assert [seg(t, s)[1] for s in range(5)] == [[-1, -2], [0.001, 4], [3 + 0.001, 4 - 3], [2 + (3 + 0.001), 2 + (4 - 3)], [1.5, 0.5]] and seg(t, 0)[0] == [1.5, 0.5]
    assert seg(t, 5) == [[6.5, 5.5], [7.5, 6.5], [8.5, 6.5], [9.5, 5.5]]                # m after z is relative to the start of the closed subpath
    assert seg(t, 6) == [[9.5, 5.5], [10.5, 4.5], [10.5, 3.5], [12.5, 5.5]]             # s: reflected handle, then (1, -2) and (3, 0) relative
    assert seg(t, 7) == [[12.5, 5.5], [13.5, 6.5], [14.5, 5.5]] and seg(t, 8) == [[14.5, 5.5], [15.5, 4.5], [16.5, 5.5]]
    assert seg(t, 9)[0] == [16.5, 5.5] and seg(t, 9)[3] == [17.5, 6.5] and seg(t, 11)[3] == [14.5, 9.5]            # a1 1 0 011 1, then a2 2 0 10-3 3
    assert [seg(t, s) for s in range(12, 16)] == [[[20, 20], [25, 20]], [[25, 20], [25, 25]], [[25, 25], [30, 25]], [[30, 25], [30, 30]]]
    m = table_of("malformed")                                                        # every path ends at its last good command
    assert [seg(m, s) for s in range(4)] == [[[10, 10], [50, 10]], [[50, 10], [50, 50]], [[60, 60], [90, 60]], [[10, 60], [40, 90]]]
    z = table_of("zero_area")
    assert [seg(z, s) for s in range(2)] == [[[10, 50], [90, 50]], [[20, 50], [95, 50]]]
    v = table_of("viewbox_only")
    assert seg(v, 0) == [[2, 2], [20, 40], [40, -20], [62, 46]] and seg(v, 1) == [[4, 1], [60, 1]]
    assert seg(v, 2) == [[60, 1], [60 + K * 3, 1], [63, 4 + K * (1 - 4)], [63, 4]] and seg(v, 8)[3] == [4, 1]
    for name in ("loop", "loop_flat"):
        q = table_of(name)
        assert seg(q, 0)[0] == seg(q, 0)[3]
    assert seg(table_of("loop"), 0) == [[5, 5], [9, 1], [9, 9], [5, 5]]


def test_parser_transforms_by_hand():
    t = table_of("transforms")

    def M(a, b, c, d, e, f): return np.array([[a, c, e], [b, d, f], [0, 0, 1.0]])
    def rot(deg): c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg)); return M(c, s, -s, c, 0, 0)
    def tr(x, y=0.0): return M(1, 0, 0, 1, x, y)
    g1 = tr(20, 30)
    g2 = g1 @ M(2, 0, 0, 0.5, 0, 0) @ tr(10)
    want = [np.eye(3), g1, g1 @ rot(30), g2, g2 @ M(1, 0.2, -0.3, 1, 5, 6), g2 @ M(1, 0, math.tan(math.radians(20)), 1, 0, 0) @ M(1, math.tan(math.radians(-10)), 0, 1, 0, 0),
            g1 @ tr(100, 100) @ rot(-45) @ tr(-100, -100), g1 @ M(-1, 0, 0, 1, 0, 0) @ tr(-200, 0) @ rot(10)]
    for m, w in zip(t.mats, want):
        assert np.allclose([m[0], m[2], m[4], m[1], m[3], m[5]], w[:2].reshape(-1), rtol=1e-14, atol=1e-12)
    assert t.mat.tolist() == [2] * 4 + [4] + [5] * 4 + [6] * 4 + [7] * 2
    raw = t.raw_mats()
    assert np.array_equal(raw[:, [0, 2, 4]], t.mats[:, [0, 2, 4]]) and np.array_equal(raw[:, [1, 3]], -t.mats[:, [1, 3]]) and np.array_equal(raw[:, 5], 300.0 - t.mats[:, 5])


def test_tokenizer_compact_forms():
    from orip.svg import tokenize_path as T
    assert T("M1.5.5-1-2 1e-3,4") == [("M", (1.5, 0.5)), ("L", (-1.0, -2.0)), ("L", (0.001, 4.0))]
    assert T("m1 2 3 4z") == [("m", (1.0, 2.0)), ("l", (3.0, 4.0)), ("z", ())]
    assert T("M0 0a1 1 0 011 1") == [("M", (0.0, 0.0)), ("a", (1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0))]
    assert T("M0 0a2 2 0 10-3 3") == [("M", (0.0, 0.0)), ("a", (2.0, 2.0, 0.0, 1.0, 0.0, -3.0, 3.0))]
    assert T("M0,0L1,1,2,2 , 3 3") == [("M", (0.0, 0.0)), ("L", (1.0, 1.0)), ("L", (2.0, 2.0)), ("L", (3.0, 3.0))]
    assert T("M-.5+.5E1h-1e+1V.0") == [("M", (-0.5, 5.0)), ("h", (-10.0,)), ("V", (0.0,))]
    assert T("M1 1L2 2L3") == [("M", (1.0, 1.0)), ("L", (2.0, 2.0))]                    # a malformed tail ends the path at the last good command
    assert T("M1 1L2 2X3 3L4 4") == [("M", (1.0, 1.0)), ("L", (2.0, 2.0))]
    assert T("L1 1M2 2") == [] and T("") == [] and T("M1") == [] and T("M1 1z5 5") == [("M", (1.0, 1.0)), ("z", ())]
    assert T("M0 0A5 5 0 2 1 8 8") == [("M", (0.0, 0.0))]                              # a flag is 0 or 1


def test_lengths_and_canvas_height():
    from orip import svg as SV
    import xml.etree.ElementTree as ET
    assert [SV.parse_length(s) for s in ("12", " 12.5px ", "210mm", "1e2%", "-.5em", "", None, "abc", "12 px")] == [12.0, 12.5, 210.0, 100.0, -0.5, None, None, None, None]
    H = lambda s: SV.canvas_height(ET.fromstring(s))
    assert H('<svg width="10" height="20mm"/>') == 20.0 and H('<svg height="33"/>') == 33.0
    assert H('<svg viewBox="0 0 64.4 48.6"/>') == 49.0 and H('<svg width="5" viewBox="0,0,10,20.5"/>') == 20.0          # int(round()): half to even
    assert H('<svg viewBox="0 0 10"/>') == 100.0 and H('<svg viewBox="0 0 a b"/>') == 100.0 and H('<svg/>') == 100.0 and H('<svg width="7"/>') == 100.0


# ------------------------------------------------------------------ arcs against their ellipses
def bezier(P, t):
    t = np.asarray(t, np.float64)[:, None]
    P = np.asarray(P, np.float64)
    if len(P) == 2: return (1 - t) * P[0] + t * P[1]
    if len(P) == 3: return (1 - t) ** 2 * P[0] + 2 * (1 - t) * t * P[1] + t ** 2 * P[2]
    return (1 - t) ** 3 * P[0] + 3 * (1 - t) ** 2 * t * P[1] + 3 * (1 - t) * t ** 2 * P[2] + t ** 3 * P[3]


def rho(P, cx, cy, rx, ry, phi=0.0):
    """radius of the points of a cubic in the frame where the ellipse is the unit circle"""
    p = bezier(P, np.linspace(0, 1, 33)) - [cx, cy]
    c, s = math.cos(phi), math.sin(phi)
    u, v = (c * p[:, 0] + s * p[:, 1]) / rx, (-s * p[:, 0] + c * p[:, 1]) / ry
    return np.hypot(u, v), np.degrees(np.unwrap(np.arctan2(v, u)))


def check_arc(t, segs, cx, cy, rx, ry, total_deg, phi=0.0):
    """every piece within 2.8e-4 r of the ellipse (the known error of the 4/3 tan(theta / 4) handles at 90 degrees), none above 90 degrees, the signed total"""
    swept = 0.0
    for s in segs:
        r, ang = rho(t.ctrl[s], cx, cy, rx, ry, phi)
        assert np.abs(r - 1.0).max() <= 2.8e-4, (s, np.abs(r - 1.0).max())
        assert abs(ang[-1] - ang[0]) <= 90.0 + 1e-6
        swept += ang[-1] - ang[0]
    assert abs(swept - total_deg) < 1e-6, swept


def test_arcs_lie_on_their_ellipses():
    t = table_of("arcs")
    h = 25.0 * math.sqrt(1.0 - (30.0 / 40.0) ** 2)               # chord 60 on radii 40 x 25: the centres lie this far above or below the chord
    small = 2.0 * math.degrees(math.asin(30.0 / 40.0))
    # y grows downwards: sweep 1 turns by positive angles, i.e. clockwise on the screen, so the small sweep-1 arc from left to right bulges upwards (centre below)
    check_arc(t, [0, 1], 80, 100 - h, 40, 25, -small)             # large 0 sweep 0
    check_arc(t, [2, 3], 180, 100 + h, 40, 25, small)             # large 0 sweep 1
    check_arc(t, [4, 5, 6], 280, 100 + h, 40, 25, -(360 - small)) # large 1 sweep 0
    check_arc(t, [7, 8, 9], 80, 220 - h, 40, 25, 360 - small)     # large 1 sweep 1
    n5 = int(t.sub_off[5] - t.sub_off[4]) - 2                     # the rotated large arc, then a half circle of radius 10 round (220, 230)
    s0 = int(t.sub_off[4])
    check_arc(t, [s0 + n5, s0 + n5 + 1], 220, 230, 10, 10, -180.0)
    assert t.ctrl[s0, 0].tolist() == [150, 220] and t.ctrl[s0 + n5 - 1, 3].tolist() == [210, 230]
    s6 = int(t.sub_off[5])
    check_arc(t, [s6, s6 + 1], 290, 220, 40, 40, 180.0)           # radii 5 on a chord of 80: scaled up to 40
    s7 = int(t.sub_off[6])
    assert seg(t, s7) == [[250, 260], [330, 260]] and seg(t, s7 + 1) == [[330, 260], [340, 270]]     # zero radius: a line; an arc to where it stands: nothing
    s8 = int(t.sub_off[7])
    check_arc(t, [s8, s8 + 1, s8 + 2, s8 + 3], 30, 20, 10, 10, 360.0)
    c = table_of("commands_abs")
    check_arc(c, [7, 8], 55, 50, 15, 10, 180.0)
    e = table_of("elements")
    check_arc(e, [26, 27, 28, 29], 160, 30, 20, 20, 360.0); check_arc(e, [30, 31, 32, 33], 160, 100, 30, 15, 360.0)
    check_arc(e, [15], 92, 55, 8, 5, 90.0)


def test_rotated_arc_on_its_ellipse():
    """M150 220 A40 20 30 1 1 210 230: the centre from the end points by the formulae of the SVG implementation notes, worked here with numpy"""
    t = table_of("arcs")
    s0, n5 = int(t.sub_off[4]), int(t.sub_off[5] - t.sub_off[4]) - 2
    phi = math.radians(30)
    R = np.array([[math.cos(phi), math.sin(phi)], [-math.sin(phi), math.cos(phi)]])
    p = R @ np.array([(150 - 210) / 2.0, (220 - 230) / 2.0])
    rx, ry = 40.0, 20.0
    lam = (p[0] / rx) ** 2 + (p[1] / ry) ** 2
    assert lam < 1
    co = math.sqrt((rx * rx * ry * ry - rx * rx * p[1] ** 2 - ry * ry * p[0] ** 2) / (rx * rx * p[1] ** 2 + ry * ry * p[0] ** 2))       # large == sweep: minus
    cp = -co * np.array([rx * p[1] / ry, -ry * p[0] / rx])
    c = R.T @ cp + [(150 + 210) / 2.0, (220 + 230) / 2.0]
    total = 0.0
    for s in range(s0, s0 + n5):
        r, ang = rho(t.ctrl[s], c[0], c[1], rx, ry, phi)
        assert np.abs(r - 1.0).max() <= 2.8e-4 and 0 < ang[-1] - ang[0] <= 90.0 + 1e-6
        total += ang[-1] - ang[0]
    assert 180.0 < total < 360.0 and n5 == math.ceil(total / 90.0)


# ------------------------------------------------------------------ fit
def test_fit_transform_against_recorded_parameters():
    from orip import svg as SV
    box = tuple(G["fit_box"].tolist())
    auto = [i for i in range(FIT_COUNT) if np.array_equal(G[f"fit_{i}_params"][:2], G[f"fit_{i}_params"][[0, 0]]) and i == FIT_COUNT - 1][0]
    assert SV.fit_transform(box, SV.SvgOptions()) == tuple(G[f"fit_{auto}_params"].tolist())
    # by hand: a 100 x 50 box at (-10, 20) on A4 with margin 10: 190 / 100 against 277 / 50
    b = (-10.0, 20.0, 90.0, 70.0)
    assert SV.fit_transform(b, SV.SvgOptions()) == (1.9, 1.9, 10.0 - -10.0 * 1.9, 10.0 - 20.0 * 1.9)
    assert SV.fit_transform(b, options_for(["--scale", "0.5"])) == (0.5, 0.5, 15.0, 0.0)
    assert SV.fit_transform(b, options_for(["--scale", "0.5", "--scale-x", "2"])) == (2.0, 0.5, 30.0, 0.0)
    assert SV.fit_transform(b, options_for(["--scale-y", "3"])) == (1.9, 3.0, 29.0, -50.0)
    assert SV.fit_transform(b, options_for(["--page-width-mm", "297", "--page-height-mm", "210", "--margin-mm", "15"])) == (2.67, 2.67, 15.0 + 10.0 * 2.67, 15.0 - 20.0 * 2.67)
    assert SV.fit_transform(b, options_for(["--page-width-mm", "10", "--margin-mm", "20"]))[0] == 1e-6 / 100.0             # avail = max(1e-6, ...)
    for deg in ((0.0, 0.0, 0.0, 5.0), (1.0, 2.0, 9.0, 2.0), (3.0, 3.0, 3.0, 3.0)):                                          # zero width or height: s = 1, o = 0
        assert SV.fit_transform(deg, options_for(["--scale", "7"])) == (1.0, 1.0, 0.0, 0.0)


@pytest.mark.parametrize("i", range(FIT_COUNT))
def test_double_fit_matches_reference_bit_for_bit(i):
    sx, sy, ox, oy = G[f"fit_{i}_params"].tolist()
    _, got = SD.fit_numpy((None, G["fit_in"]), sx, sy, ox, oy)
    want = G[f"fit_{i}_out"]
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    assert SD.bbox_numpy((None, G["fit_in"])) == tuple(G["fit_box"].tolist())


def test_fit_families_are_in_the_fixture():
    v = G["fit_in"][:, 0]
    assert 5e-05 in v and (v < 0).any() and ((np.abs(v) < 1e-4) & (v != 0)).sum() > 500
    assert all(j / 32.0 in v for j in range(-399, 400, 2)) and all(k / 1e4 + 5e-5 in v for k in range(-300, 301))
    out = G["fit_0_out"][:, 0]                                                     # s = 1, o = 0: the trap and the genuine ties, as the reference rounds them
    assert out[v == 5e-05][0] == 0.0001 and out[v == -5e-05][0] == -0.0001
    assert out[v == 1 / 32.0][0] == 0.0312 and out[v == 3 / 32.0][0] == 0.0938 and out[v == 5 / 32.0][0] == 0.1562       # .03125 -> even 312, .09375 -> even 938


# ------------------------------------------------------------------ the chord contract
@pytest.mark.parametrize("i", range(len(RUNS)))
def test_chord_contract(i):
    """every curve, 32 parameters inside each piece: |B(t) - chord(t)| in page mm, with the scale that was applied, stays within tolerance_mm (+ 1e-9 of the
    box diagonal for rounding).  B from the ORIGINAL control points (Bernstein form) and the matrix; the chord from the double's points."""
    from orip import svg as SV
    name, key = RUNS[i]
    t = table_of(name)
    o = options_for(ARGS[key])
    rec = G[f"run_{i}_fit"]
    sx, sy, tol_raw = float(rec[0]), float(rec[1]), float(rec[8])
    if t.n_seg == 0:
        return
    tol = SV.tolerance_mm(o)
    assert max(abs(sx), abs(sy)) * tol_raw <= tol * (1 + 1e-12)
    off, pts = SD.flatten_numpy(t, tol_raw)
    box = SD.bbox_numpy((off, pts))
    assert box == tuple(rec[4:8].tolist()) and SV.fit_transform(box, o)[:2] == (sx, sy)
    diag = math.hypot((box[2] - box[0]) * sx, (box[3] - box[1]) * sy)
    n = SD.piece_counts(t.kind, SD.transform(t), tol_raw)
    m = t.raw_mats()[t.mat]
    sub = np.repeat(np.arange(t.n_sub), np.diff(t.sub_off))
    first = np.concatenate([[0], np.cumsum(n)])[:-1] + sub                      # index of the segment's point 0
    u = (np.arange(32) + 0.5) / 32.0
    worst = 0.0
    for s in np.nonzero(t.kind >= 2)[0]:
        P = t.ctrl[s, :t.kind[s] + 1]
        for j in range(int(n[s])):
            B = bezier(P, (j + u) / n[s])
            Bx, By = m[s, 0] * B[:, 0] + m[s, 2] * B[:, 1] + m[s, 4], m[s, 1] * B[:, 0] + m[s, 3] * B[:, 1] + m[s, 5]
            a, b = pts[first[s] + j], pts[first[s] + j + 1]
            cx, cy = a[0] + (b[0] - a[0]) * u, a[1] + (b[1] - a[1]) * u
            worst = max(worst, float(np.hypot((Bx - cx) * sx, (By - cy) * sy).max()))
    assert worst <= tol + 1e-9 * diag, (worst, tol)
    if (t.kind >= 2).any() and min(abs(sx), abs(sy)) * tol_raw > 0.5 * tol:
        assert worst > 0.01 * tol                                                  # and the pieces are not absurdly fine either


def test_tolerance_bound_holds_before_any_curve_is_cut():
    """the applied scale never exceeds the bound taken from the end points; only the two drawings whose end points all coincide needed a second flattening"""
    from orip import svg as SV
    for i, (name, key) in enumerate(RUNS):
        t = table_of(name)
        if t.n_seg == 0:
            continue
        rec = G[f"run_{i}_fit"]
        o = options_for(ARGS[key])
        if name not in ("loop", "loop_flat"):
            assert int(rec[9]) == 1 and max(abs(rec[0]), abs(rec[1])) <= SV.tolerance_bound(t, o) * (1 + 1e-12), (name, key)
            assert rec[8] == SV.tolerance_mm(o) / SV.tolerance_bound(t, o)
        else:
            assert int(rec[9]) >= 1


# ------------------------------------------------------------------ the whole host path
@pytest.mark.parametrize("i", range(len(RUNS)))
def test_host_path_reproduces_reference_stream(i):
    from orip import svg as SV, gcode as GC
    name, key = RUNS[i]
    data, info = SV.build_stream_from_svg(svg_text(name), options_for(ARGS[key]), want_paths=True, **SD.svg_doubles())
    want = bytes(G[f"run_{i}_bin"])
    assert len(data) == len(want) and data == want, (name, key)
    off, pts = info["fitted_paths"]
    assert np.array_equal(off, G[f"run_{i}_off"]) and pts.tobytes() == G[f"run_{i}_pts"].tobytes()
    text = SV.gcode_text(off, pts)
    assert text.encode() == bytes(G[f"run_{i}_gcode"])
    off2, pts2, _ = GC.parse_gcode(text)                                           # the reference's parser rules (tests/test_gcode_host.py) read the paths back exactly
    keep = np.diff(off) >= 2
    assert np.array_equal(off2, np.concatenate([[0], np.cumsum(np.diff(off)[keep])])) and np.array_equal(pts2, pts[np.repeat(keep, np.diff(off))])
    data2, _ = SV.build_stream_from_svg(svg_text(name), options_for(ARGS[key]), **SD.svg_doubles())      # without the points fetched
    assert data2 == want


def test_gcode_text_dialect():
    from orip.svg import gcode_text
    off = np.array([0, 2, 5]); pts = np.array([[1.0, 2.0], [3.5, -0.0001], [0.0, 0.0], [10.12345, 5.0], [1e3, 2.5]])
    assert gcode_text(off, pts) == "G21\nG90\nM5\nG0 X1.0000 Y2.0000\nM3\nG1 X3.5000 Y-0.0001\nM5\nG0 X0.0000 Y0.0000\nM3\nG1 X10.1235 Y5.0000\nG1 X1000.0000 Y2.5000\nM5\n"
    assert gcode_text(np.array([0]), np.zeros((0, 2))) == "G21\nG90\nM5\n"
    assert gcode_text(off[:2], pts[:2], passes=2).count("M3") == 2


def test_options_and_command_lines():
    from orip import svg as SV
    d = SV.SvgOptions()
    assert (d.output, d.movement_speed, d.cutting_speed, d.passes, d.pass_depth, d.page_width_mm, d.page_height_mm, d.margin_mm, d.scale, d.scale_x, d.scale_y) == \
        ("from_svg.gcode", 8000.0, 2000.0, 1, 0.0, 210.0, 297.0, 10.0, None, None, None)
    assert (d.output_stream, d.gcode_output, d.steps_per_mm, d.target_width_steps, d.target_height_steps, d.invert_y, d.color_index, d.speed_scale, d.no_reorder, d.no_preview,
            d.preview_render_width, d.preview_render_height, d.tolerance_mm) == (None, None, 40.0, None, None, 0, 3, 1.0, False, False, 1200, 900, None)
    assert SV.tolerance_mm(d) == 0.0125 and SV.tolerance_mm(options_for(["--steps-per-mm", "10"])) == 0.05 and SV.tolerance_mm(options_for(["--tolerance-mm", "0.3"])) == 0.3
    with pytest.raises(ValueError):
        SV.tolerance_mm(options_for(["--tolerance-mm", "0"]))
    a = SV.build_gcode_argparser().parse_args(["x.svg", "--movement-speed", "1", "--cutting-speed", "2", "--passes", "3", "--pass-depth", "0.5", "--scale", "2"])
    o = SV.options_from_args(a)
    assert (o.passes, o.scale, o.output) == (3, 2.0, "from_svg.gcode")
    g = SV.gcode_options(options_for(["--steps-per-mm", "12.5", "--page-width-mm", "100", "--invert-y", "1", "--color-index", "5", "--speed-scale", "2", "--no-reorder"]))
    assert (g.target_width_steps, g.target_height_steps, g.scale_x, g.scale_y, g.offset_x_mm, g.offset_y_mm, g.invert_y, g.color_index, g.speed_scale, g.no_reorder) == \
        (1250, 3712, 1.0, 1.0, 0.0, 0.0, 1, 5, 2.0, True)
    g = SV.gcode_options(options_for(["--target-width-steps", "300"]))               # one size alone: the page rules
    assert (g.target_width_steps, g.target_height_steps) == (8400, 11880)
    g = SV.gcode_options(options_for(["--target-width-steps", "300", "--target-height-steps", "200"]))
    assert (g.target_width_steps, g.target_height_steps) == (300, 200)


def test_double_refuses_what_the_device_refuses():
    from orip.svg import SegmentTable
    def T(ctrl, kind=2):
        return SegmentTable(np.array([kind], np.int32), np.array(ctrl, np.float64).reshape(1, 4, 2), np.zeros(1, np.int32), np.array([0, 1], np.int64), np.zeros(1, np.uint8),
                            np.array([[1.0, 0, 0, -1.0, 0, 0]]), 0.0)
    with pytest.raises(ValueError):
        SD.flatten_numpy(T([0, 0, 0, 0, 1e12, 0, 1e12, 0]), 1e-3)                     # more than 2^16 pieces
    with pytest.raises(ValueError):
        SD.flatten_numpy(T([0, 0, np.inf, 0, 1, 0, 1, 0]), 1.0)
    with pytest.raises(ValueError):
        SD.flatten_numpy(T([0, 0, 1, 1, 2, 0, 2, 0]), 0.0)
    off, pts = SD.flatten_numpy(T([0, 0, 0, 0, 16, 0, 16, 0]), 0.25)                  # |d| = 16 = n^2 k with k = 1: exactly on the boundary, n = 4
    assert len(pts) == 5 and pts[:, 0].tolist() == [0.0, 1.0, 4.0, 9.0, 16.0]
    off, pts = SD.flatten_numpy(T([0, 0, 0, 0, np.nextafter(16, 17), 0, np.nextafter(16, 17), 0]), 0.25)
    assert len(pts) == 6
    with pytest.raises(ValueError):
        SD.fit_numpy((off, pts), 1e9, 1.0, 0.0, 0.0)


def test_scripts_without_gpu_fail_loudly_or_match(tmp_path):
    """the scripts have no CPU path: without a usable GPU they exit non-zero and write nothing; with one they write the recorded bytes"""
    src = tmp_path / "d.svg"; src.write_bytes(bytes(G["svg_commands_abs"]))
    i = RUNS.index(["commands_abs", "coarse"])
    d = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
    r = subprocess.run([sys.executable, os.path.join(d, "svg2stream.py"), str(src), "--no-preview"] + ARGS["coarse"], capture_output=True, text=True, timeout=300)
    if r.returncode == 0:
        assert (tmp_path / "d_stream.bin").read_bytes() == bytes(G[f"run_{i}_bin"]) and (tmp_path / "d.gcode").read_bytes() == bytes(G[f"run_{i}_gcode"])
    else:
        assert "no CPU fallback" in r.stderr and not (tmp_path / "d_stream.bin").exists() and not (tmp_path / "d.gcode").exists()
    r = subprocess.run([sys.executable, os.path.join(d, "svg2gcode.py"), str(src), "-o", str(tmp_path / "o.gcode"), "--steps-per-mm", "10"], capture_output=True, text=True, timeout=300)
    if r.returncode == 0:
        assert (tmp_path / "o.gcode").read_bytes() == bytes(G[f"run_{i}_gcode"])
    else:
        assert "no CPU fallback" in r.stderr and not (tmp_path / "o.gcode").exists()
    r = subprocess.run([sys.executable, os.path.join(d, "svg2stream.py"), str(tmp_path / "missing.svg")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "not found" in r.stderr
