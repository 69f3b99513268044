"""--clip on the host, without a GPU: the sequential double (tests/clip_double.py) against the invariants of the rule that need no second opinion, on every
crafted shape and on the random drawing -- every point inside the rectangle, no stroke under two points or with a repeated neighbour, the sources ascending,
the counts adding up, a reversed path giving the reversed strokes, an input inside the rectangle giving orip_gcode_to_steps' result -- and a few cuts worked
out by hand; the option checks and the parsers of both tools; and the host flow of both tools with every device step injected as a double: on a drawing
inside the sheet nothing changes, off the sheet the line along the border is gone, and the option works with the others.  No comparison has a tolerance."""
import numpy as np
import pytest

import clip_cases as CC
import clip_double as CD
import gcode_double as D
import merge_cases as MC
import pens_double as PD

SMALL = CC.small_cases()
CASES = dict(SMALL, random=CC.random_case())


def never(*a, **k):
    raise AssertionError("the clip was called without --clip")


def strokes(off, pts):
    return [list(map(tuple, pts[a:b].tolist())) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]


def path_strokes(out, n):
    """per input path the strokes it became"""
    off, pts, src, _ = out
    per = [[] for _ in range(n)]
    for s, p in zip(strokes(off, pts), src.tolist()):
        per[p].append(s)
    return per


# ------------------------------------------------------------------ the rule, on the double
@pytest.mark.parametrize("name", sorted(CASES))
def test_invariants(name):
    off_mm, pts_mm, m, rect = CASES[name]
    n = len(off_mm) - 1
    out = off, pts, src, st = CD.clip_numpy(off_mm, pts_mm, m, rect)
    k = len(off) - 1
    assert off.dtype == np.int64 and pts.dtype == np.int32 and src.dtype == np.int32 and off[0] == 0 and int(off[-1]) == len(pts) and len(src) == k
    x0, y0, x1, y1 = rect
    assert ((pts[:, 0] >= x0) & (pts[:, 0] <= x1) & (pts[:, 1] >= y0) & (pts[:, 1] <= y1)).all()
    assert (np.diff(off) >= 2).all()
    same = (np.diff(pts, axis=0) == 0).all(1); same[off[1:-1] - 1] = False
    assert not same.any()
    assert (np.diff(src) >= 0).all() and (k == 0 or (0 <= src[0] and src[-1] < n))
    lens = np.diff(off_mm)
    assert st["segments"] == int((lens - 1).clip(0).sum()) == st["inside"] + st["cut"] + st["outside"] and st["paths_out"] == k and st["points_out"] == len(pts)
    assert set(st) == set(CD.STATS)
    # every path back to front: the same strokes, back to front
    rev_pts = np.concatenate([pts_mm[a:b][::-1] for a, b in zip(off_mm[:-1], off_mm[1:])] + [np.zeros((0, 2))])
    back = CD.clip_numpy(off_mm, rev_pts, m, rect)
    assert [[s[::-1] for s in per[::-1]] for per in path_strokes(out, n)] == path_strokes(back, n)
    assert {q: st[q] for q in ("segments", "inside", "cut", "outside")} == {q: back[3][q] for q in ("segments", "inside", "cut", "outside")}
    # the paths that lie inside the rectangle with every point are what orip_gcode_to_steps makes of them
    x, y = CD.unclamped_steps(pts_mm, m)
    ok = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    whole = [p for p in range(n) if lens[p] >= 2 and ok[off_mm[p]:off_mm[p + 1]].all()]
    sub_off = np.concatenate([[0], np.cumsum(lens[whole])]).astype(np.int64)
    sub_pts = np.concatenate([pts_mm[off_mm[p]:off_mm[p + 1]] for p in whole] + [np.zeros((0, 2))])
    w_off, w_pts = D.to_steps_numpy(sub_off, sub_pts, m)
    mine = [s for p in whole for s in path_strokes(out, n)[p]]
    assert mine == strokes(w_off, w_pts)


def test_inside_the_sheet_it_is_the_conversion():
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 7, 400)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pts = rng.integers(0, 17, (int(off[-1]), 2)) * 0.25                    # 0 .. 4 mm at 2 steps per mm: steps 0 .. 8, halves rounded to even, many repeats
    for inv in (0, 1):
        m = CC.sheet_map(9, 9, 2.0, invert_y=inv)
        S = PD.StepsWithSource()
        w_off, w_pts = S.steps(off, pts, m)
        g_off, g_pts, g_src, st = CD.clip_numpy(off, pts, m, CD.sheet(m))
        assert np.array_equal(g_off, w_off) and np.array_equal(g_pts, w_pts) and np.array_equal(g_src, S.src) and 50 < len(w_off) < 400
        assert st["cut"] == st["outside"] == 0 and st["inside"] == st["segments"]


def test_the_random_case_is_a_real_test():
    off, pts, src, st = CD.clip_numpy(*CASES["random"])
    assert st["inside"] > 100 and st["cut"] > 100 and st["outside"] > 100 and st["paths_out"] != len(CASES["random"][0]) - 1
    assert (np.diff(src) == 0).sum() > 20                                  # paths that became several strokes
    x, y = CD.unclamped_steps(CASES["random"][1], CASES["random"][2])
    assert ((CASES["random"][1] * 2.0) % 1.0 == 0.5).any()                 # halves in the conversion


def test_cuts_worked_out_by_hand():
    def one(*path, rect=(0, 0, 7, 7), m=None):
        o, p, s, st = CD.clip_numpy(*CC.case([list(path)], m, rect))
        return strokes(o, p)
    assert one((3, 3), (10, 5)) == [[(3, 3), (7, 4)]]                      # x = 7 at t = 4/7: y = 3 + 8/7
    assert one((10, 5), (3, 3)) == [[(7, 4), (3, 3)]]
    assert one((-2, 2), (10, 6)) == [[(0, 3), (7, 5)]]                     # y = 2 + 2/3 and y = 5
    assert one((-1, 2), (1, 3)) == [[(0, 3), (1, 3)]] and one((-1, 3), (1, 2)) == [[(0, 3), (1, 2)]]      # 2.5 from below and from above: both up
    assert one((3, -1), (4, 1)) == [[(4, 0), (4, 1)]] and one((6, 1), (8, 0)) == [[(6, 1), (7, 1)]]
    assert one((-2, -2), (3, 3)) == [[(0, 0), (3, 3)]] and one((5, 9), (9, 5)) == [] and one((-1, 1), (3, -2)) == []
    assert one((-2, 0), (10, 0)) == [[(0, 0), (7, 0)]] and one((-2, -1), (10, -1)) == []
    assert one((2, 2), (7, 4), (10, 4), (7, 4), (2, 6)) == [[(2, 2), (7, 4)], [(7, 4), (2, 6)]]
    assert one((2, 2), (2, 2), (5, 5), (5, 5), (9, 9), (9, 9), (5, 6)) == [[(2, 2), (5, 5), (7, 7)], [(6, 7), (5, 6)]]      # (9, 9) -> (5, 6) comes in through y = 7 at x = 6 1/3
    T = CC.TOP
    assert one((-T, -T + 1), (T, T)) == [[(0, 1), (7, 7)]]                 # y = x + 1/2 + x / 2^31 along the sheet: (0, 1/2) up, and out through (6 1/2, 7)
    o, p, s, st = CD.clip_numpy(*SMALL["path_zigzag"])
    assert s.tolist() == [0, 1, 1, 1, 1, 1, 2] and np.diff(o).tolist() == [2, 2, 3, 3, 3, 2, 2]
    with pytest.raises(CD.RangeError):
        CD.clip_numpy(*CC.range_error_case())
    with pytest.raises(OverflowError):
        CD.clip_numpy(*CC.case([[(1, 1), (float("inf"), 2)]]))
    assert CD.clip_numpy(*CC.case([[(1, 1), (2, 2)], [(float("nan"), 2)]]))[3]["paths_out"] == 1      # a lone point is not looked at, as in the conversion


# ------------------------------------------------------------------ the command lines
def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def test_options_parse_on_both_tools():
    from orip import svg as SV, gcode as GC
    assert GC.GcodeOptions().clip is False and GC.GcodeOptions().clip_margin_mm is None and SV.SvgOptions().clip is False and SV.SvgOptions().clip_margin_mm is None
    a = GC.build_argparser().parse_args(["in.gcode"])
    assert a.clip is False and a.clip_margin_mm is None and SV.build_stream_argparser().parse_args(["in.svg"]).clip is False
    o = GC.options_from_args(GC.build_argparser().parse_args(["in.gcode", "--clip", "--clip-margin-mm", "2.5"]))
    assert o.clip is True and o.clip_margin_mm == 2.5 and GC.clip_rect(o) == (100, 100, 8400 - 1 - 100, 11880 - 1 - 100)
    assert GC.clip_rect(GC.GcodeOptions(clip=True)) == (0, 0, 8399, 11879) and GC.clip_rect(GC.GcodeOptions()) is None
    assert GC.clip_rect(GC.GcodeOptions(clip=True, clip_margin_mm=0.0125)) == (0, 0, 8399, 11879)          # half a step rounds to even
    assert GC.clip_rect(GC.GcodeOptions(clip=True, clip_margin_mm=1.0, steps_per_mm=3.0, target_width_steps=7, target_height_steps=9)) == (3, 3, 3, 5)
    s = svg_options(["--clip", "--clip-margin-mm", "1", "--steps-per-mm", "10", "--page-width-mm", "50", "--page-height-mm", "40"])
    assert s.clip is True and SV.gcode_options(s).clip is True and GC.clip_rect(SV.gcode_options(s)) == (10, 10, 489, 389)
    assert SV.gcode_options(SV.SvgOptions()).clip is False and SV.gcode_options(SV.SvgOptions()).clip_margin_mm is None
    assert not hasattr(SV.build_gcode_argparser().parse_args(["in.svg"]), "clip")          # svg2gcode.py writes G-code: the clip lives in the stream


def test_option_errors():
    from orip import gcode as GC, svg as SV
    text = CC.inside_gcode()
    bad = (GC.GcodeOptions(clip_margin_mm=1.0), GC.GcodeOptions(clip_margin_mm=0.0), GC.GcodeOptions(clip=True, clip_margin_mm=-0.5), GC.GcodeOptions(clip=True, clip_margin_mm=float("nan")),
           GC.GcodeOptions(clip=True, clip_margin_mm=float("inf")), GC.GcodeOptions(clip=True, clip_margin_mm=105.0),
           GC.GcodeOptions(clip=True, clip_margin_mm=1.0, steps_per_mm=3.0, target_width_steps=6, target_height_steps=9))
    for o in bad:
        with pytest.raises(ValueError):
            GC.clip_rect(o)
        with pytest.raises(ValueError):
            GC.build_stream_from_gcode(text, o, **dict(CD.gcode_doubles(), clip_fn=never, steps_fn=never))
    for args in (["--clip-margin-mm", "1"], ["--clip", "--clip-margin-mm", "-1"], ["--clip", "--clip-margin-mm", "200"]):
        with pytest.raises(ValueError):
            SV.build_stream_from_svg(CC.TOOL_SVG, svg_options(args), **dict(CD.svg_doubles(), clip_fn=never, steps_fn=never))
    with pytest.raises(ValueError):
        GC.main(["nowhere.gcode", "--clip-margin-mm", "3"])                                # before the file is looked for


# ------------------------------------------------------------------ the host flow through the doubles
def border_steps(data, column=0, axis=0):
    """pen-down steps of a stream that run along x = column (axis 1: along y = column): both ends on it"""
    return sum(1 for _, s in MC.strokes_of(data) for a, b in zip(s[:-1], s[1:]) if a[axis] == column and b[axis] == column)


def test_off_by_default_and_bytes_unchanged():
    from orip import gcode as GC, svg as SV
    from test_gcode_host import G, MAIN_CASES, options_for
    plain = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=CD.gcode_doubles()["codes_fn"], pack_fn=D.pack_numpy)
    for i, (name, args) in enumerate(MAIN_CASES):
        data, info = GC.build_stream_from_gcode(bytes(G[f"text_{name}"]), options_for(args), clip_fn=never, **plain)
        assert data == bytes(G[f"main_{i}_bin"]) and "clip" not in info
    a = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS), **PD.pens_doubles())
    b = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS), clip_fn=never, **PD.pens_doubles())
    assert a[0] == b[0] and "clip" not in b[1]


@pytest.mark.parametrize("extra", [{}, {"tool_pens": True}, {"tool_pens": True, "allow_reverse": True, "merge_paths": True, "improve_order": True}, {"clip_margin_mm": 2.0}])
def test_gcode_inside_the_sheet_nothing_changes(extra):
    from orip import gcode as GC
    text = CC.inside_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(**{k: v for k, v in extra.items() if k != "clip_margin_mm"}), **dict(CD.gcode_doubles(), clip_fn=never))
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(clip=True, **extra), **dict(CD.gcode_doubles(), steps_fn=never))
    c = info.pop("clip")
    assert data == plain and info == pinfo
    assert c["cut"] == c["outside"] == 0 and c["inside"] == c["segments"] == 8 and c["paths_out"] == 5 and c["points_out"] == 13
    assert c["rect"] == ((80, 80, 8319, 11799) if extra.get("clip_margin_mm") else (0, 0, 8399, 11879))


def test_gcode_circle_half_off_the_sheet():
    from orip import gcode as GC
    text = CC.circle_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(), **dict(CD.gcode_doubles(), clip_fn=never))
    K = CD.gcode_doubles()
    tm = {}
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(clip=True), timings=tm, **dict(K, steps_fn=never))
    assert border_steps(plain) > 2000 and border_steps(data) == 0                          # 80 mm of border at 40 steps per mm, drawn by the clamp alone
    c = info["clip"]
    assert c["segments"] == 94 and c["outside"] > 30 and c["cut"] == 2 and c["inside"] + c["cut"] + c["outside"] == 94 and c["paths_out"] == info["paths"] == 3 and "to_steps" in tm
    got = MC.strokes_of(data)
    assert len(got) == 3 and all(0 <= x <= 8399 and 0 <= y <= 11879 for _, s in got for x, y in s)
    assert sorted(s[0][0] for _, s in got) == [0, 1600, 4000] and sum(1 for _, s in got if s[-1][0] == 0) == 1      # the circle's two arcs start and end on the border
    assert info["steps"] < pinfo["steps"]
    # a margin moves the cut inward
    d2, i2 = GC.build_stream_from_gcode(text, GC.GcodeOptions(clip=True, clip_margin_mm=5.0), **dict(CD.gcode_doubles(), steps_fn=never))
    assert i2["clip"]["rect"] == (200, 200, 8199, 11679) and min(x for _, s in MC.strokes_of(d2) for x, _ in s) == 200 and border_steps(d2, 200) == 0


def test_gcode_clip_with_the_other_options():
    """a path that leaves the sheet and comes back, in two pens: the strokes of one path keep its pen, meet end to end only where the rule says, and the order
    and its improvement see the cut strokes"""
    from orip import gcode as GC
    lines = ["G21 G90 M5"]
    paths = [(1, [(20, 20), (-10, 30), (20, 40), (-10, 50), (20, 60)]), (2, [(30, 100), (-20, 100)]), (1, [(50, 50), (60, 60)]), (2, [(0, 100), (0, 150), (40, 150)]),
             (1, [(-5, 5), (-5, 200)])]
    for t, s in paths:
        lines += ["T%d" % t, "G0 X%g Y%g" % s[0], "M3"] + ["G1 X%g Y%g" % q for q in s[1:]] + ["M5"]
    text = "\n".join(lines) + "\n"
    base = dict(clip=True, tool_pens=True)
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(**base), **dict(CD.gcode_doubles(), steps_fn=never))
    assert info["clip"]["paths_out"] == info["paths"] == 3 + 1 + 1 + 1 and info["pens"]["paths"][:3] == [0, 4, 2] and info["clip"]["outside"] == 1
    assert sorted(c for c, _ in MC.strokes_of(data)) == [1, 1, 1, 1, 2, 2] and border_steps(data) == 50 * 40      # the stroke that IS on the border stays
    # (0, 100) ends one stroke of pen 2 and starts another: they merge; the strokes of pen 1 never touch
    d2, i2 = GC.build_stream_from_gcode(text, GC.GcodeOptions(merge_paths=True, **base), **dict(CD.gcode_doubles(), steps_fn=never))
    assert i2["merge"] == {"paths_in": 6, "paths_out": 5, "joins": 1, "cycles": 0} and len(MC.strokes_of(d2)) == 5
    d3, i3 = GC.build_stream_from_gcode(text, GC.GcodeOptions(allow_reverse=True, **base), **dict(CD.gcode_doubles(), steps_fn=never))
    d4, i4 = GC.build_stream_from_gcode(text, GC.GcodeOptions(allow_reverse=True, improve_order=True, merge_paths=True, **base), **dict(CD.gcode_doubles(), steps_fn=never))
    assert i3["clip"] == info["clip"] == i4["clip"] and i4["improve"]["travel_after"] <= i4["improve"]["travel_before"] and i4["merge"]["joins"] == 1
    down = lambda d: sum(len(s) - 1 for _, s in MC.strokes_of(d))
    assert down(data) == down(d2) == down(d3) == down(d4)                                  # the same ink every time


def test_svg_flow_clips_hatch_lines_and_keeps_their_pens():
    from orip import svg as SV
    args = CC.TOOL_SVG_ARGS + ["--pen-colors", "#f00,#0f0,#00f", "--hatch-spacing-mm", "2.0", "--hatch-inset-mm", "0"]
    plain, pinfo = SV.build_stream_from_svg(CC.TOOL_SVG, svg_options([a for a in args if a != "--clip"]), want_paths=True, **dict(CD.svg_doubles(), clip_fn=never))
    data, info = SV.build_stream_from_svg(CC.TOOL_SVG, svg_options(args), want_paths=True, **dict(CD.svg_doubles(), steps_fn=never))
    c = info["clip"]
    assert c["rect"] == (0, 0, 999, 999) and c["cut"] >= 20 and c["outside"] >= 10 and c["inside"] >= 20 and info["hatch"] == pinfo["hatch"] and info["hatch"]["segments"] > 10
    assert np.array_equal(info["fitted_paths"][1], pinfo["fitted_paths"][1]) and np.array_equal(info["path_pens"], pinfo["path_pens"])      # the G-code does not know of the clip
    got, was = MC.strokes_of(data), MC.strokes_of(plain)
    assert all(0 <= x <= 999 and 0 <= y <= 999 for _, s in got for x, y in s)
    # the clamp draws along the right and the upper edge; what is left there after the cut are the last steps of steep strokes that end on the edge
    assert border_steps(plain, 999) > 1000 and border_steps(data, 999) < 10 and border_steps(plain, 999, 1) > 100 and border_steps(data, 999, 1) < 10
    hatch_cut = [s for col, s in got if col == 2 and len(s) > 1 and s[0][1] == s[-1][1] and max(s[0][0], s[-1][0]) == 999]
    assert len(hatch_cut) > 5                                                               # blue hatch lines that now start on the edge of the sheet
    assert set(col for col, _ in got) == {0, 1, 2} and info["pens"]["paths"][:3] != pinfo["pens"]["paths"][:3]
    # with everything else on
    d2, i2 = SV.build_stream_from_svg(CC.TOOL_SVG, svg_options(args + ["--merge-paths", "--allow-reverse", "--improve-order"]), **dict(CD.svg_doubles(), steps_fn=never))
    assert i2["clip"] == c and i2["merge"]["paths_in"] == c["paths_out"] and i2["improve"]["travel_after"] <= i2["improve"]["travel_before"]
    assert sum(len(s) - 1 for _, s in MC.strokes_of(d2)) == sum(len(s) - 1 for _, s in got)


def test_svg_inside_the_page_nothing_changes():
    from orip import svg as SV
    plain, pinfo = SV.build_stream_from_svg(CC.TOOL_SVG, svg_options(CC.TOOL_SVG_INSIDE_ARGS), **dict(CD.svg_doubles(), clip_fn=never))
    data, info = SV.build_stream_from_svg(CC.TOOL_SVG, svg_options(CC.TOOL_SVG_INSIDE_ARGS + ["--clip"]), **dict(CD.svg_doubles(), steps_fn=never))
    c = info.pop("clip")
    assert data == plain and info == pinfo and c["cut"] == c["outside"] == 0 and c["inside"] > 0


def test_the_tools_print_the_clip_line(tmp_path, capsys):
    from orip import gcode as GC, svg as SV
    (tmp_path / "c.gcode").write_text(CC.circle_gcode())
    GC.main([str(tmp_path / "c.gcode"), "-o", str(tmp_path / "c.bin"), "--clip"], **dict(CD.gcode_doubles(), steps_fn=never))
    out = capsys.readouterr().out
    assert "[gcode] clip: 94 segments: " in out and " cut, " in out and "-> 3 strokes" in out and "[0, 8399] x [0, 11879]" in out
    (tmp_path / "d.svg").write_bytes(CC.TOOL_SVG)
    SV.main_stream([str(tmp_path / "d.svg"), "--no-preview"] + CC.TOOL_SVG_ARGS, **dict(CD.svg_doubles(), steps_fn=never))
    assert "[svg] clip: " in capsys.readouterr().out and (tmp_path / "d_stream.bin").exists()
