"""The pens on the host, without a GPU: the brute-force double against every order the reference's order_paths_nearest returned, the planner's events against
every call sequence its draw_color_group made (tests/golden/golden_pens.npz); stroke and fill parsing, every colour syntax, the nearest pen and its ties; T
words in and out of G-code; the command lines' defaults; and, with no new option, the bytes of the existing golden files through the doubles."""
import numpy as np
import pytest

from util import load
import pens_double as PD
import gcode_double as D
import hatch_double as HD
import svg_double as SD
from stream_double import codes_numpy

GP = load("golden_pens.npz")
ORDER_CASES = sorted(k[4:-5] for k in GP.files if k.startswith("ord_") and k.endswith("_ends"))
DCG_CASES = sorted(k[4:-4] for k in GP.files if k.startswith("dcg_") and k.endswith("_off"))


def stream_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def svg(body, attrs=""):
    return f'<svg xmlns="http://www.w3.org/2000/svg" width="100" height="100" {attrs}>{body}</svg>'


# ------------------------------------------------------------------ the double and the planner against the reference
def test_cases_are_all_there():
    assert set(ORDER_CASES) == {"uniform", "ties", "closed", "start", "ties_start"} and set(DCG_CASES) == {"random", "empty_group", "touching", "last_only"}


@pytest.mark.parametrize("name", ORDER_CASES)
def test_double_matches_reference_order(name):
    ends = GP[f"ord_{name}_ends"]
    o, r = PD.order_pens_numpy(ends, np.zeros(len(ends), int), 1, True, GP[f"ord_{name}_start"])
    assert np.array_equal(o, GP[f"ord_{name}_order"]) and np.array_equal(r, GP[f"ord_{name}_rev"])


def test_double_without_groups_is_the_old_double():
    ends = GP["ord_ties_ends"]
    o, r = PD.order_pens_numpy(ends, np.zeros(len(ends), int), 1)
    assert np.array_equal(o, D.order_numpy(ends)) and not r.any()


def test_double_key_holds_the_largest_distance():
    """corner to corner of the coordinate range is 2^31: by hand, path 0 forward (2^30 against 2^30 + 5), then path 1 by its far end (2^30 - 7 against 2^30 - 5)"""
    top = 1 << 30
    o, r = PD.order_pens_numpy([[top, 0, top, top], [top, 5, top, 7]], [0, 0], 1, True)
    assert o.tolist() == [0, 1] and r.tolist() == [False, True]


@pytest.mark.parametrize("name", DCG_CASES)
def test_planner_matches_draw_color_group(name):
    from orip import gcode as GC, stream as ST
    off, pts, pen = GP[f"dcg_{name}_off"].astype(np.int64), GP[f"dcg_{name}_pts"], GP[f"dcg_{name}_pen"]
    ends = np.concatenate([pts[off[:-1]], pts[off[1:] - 1]], 1)
    order, rev = PD.order_pens_numpy(ends, pen, 4, True)
    noff, npts = GC.gather_paths(off, pts, order, rev)
    P = GC.plan_pens(noff, npts, pen[order], [ST.PEN_UP, 0x40 | 28], ST.StreamConfig())
    assert P.kind[:2].tolist() == [ST.PEN_UP, 0x40 | 28]
    assert np.array_equal(PD.plan_events(P, skip=2), GP[f"dcg_{name}_events"])


def test_gather_reverses():
    from orip import gcode as GC
    off = np.array([0, 2, 5, 7]); pts = np.arange(14).reshape(7, 2)
    noff, npts = GC.gather_paths(off, pts, [1, 2, 0], [True, False, True])
    assert noff.tolist() == [0, 3, 5, 7] and npts[:, 0].tolist() == [8, 6, 4, 10, 12, 2, 0]
    noff, npts = GC.gather_paths(off, pts, [2, 0, 1])
    assert npts[:, 0].tolist() == [10, 12, 0, 2, 4, 6, 8]


# ------------------------------------------------------------------ colours
def test_color_syntax():
    from orip.svg import parse_color, NO_COLOR, COLOR_KEYWORDS
    assert parse_color("#f80") == (255, 136, 0) and parse_color("#FF8000") == (255, 128, 0) and parse_color(" #0a0B0c ") == (10, 11, 12)
    assert parse_color("rgb(1, 2,3)") == (1, 2, 3) and parse_color("RGB( 300 , -4 , 255 )") == (255, 0, 255)
    assert parse_color("rgb(100%, 50%, 0%)") == (255, 128, 0) and parse_color("rgb(12.5%,0%,200%)") == (32, 0, 255)
    assert len(COLOR_KEYWORDS) == 17 and parse_color("Orange") == (255, 165, 0) and parse_color("LIME") == (0, 255, 0) and parse_color("green") == (0, 128, 0)
    for word in ("none", "transparent", "currentColor", "url(#grad)", "chartreuse", "", "#12", "#12345", "#ggg", "rgb(1,2)", "rgb(1%,2,3)", "rgb(1.5,2,3)", None):
        assert parse_color(word) == NO_COLOR, word


def test_pen_colors_option():
    from orip.svg import parse_pen_colors
    from orip.stream_preview import DEFAULT_PALETTE
    assert parse_pen_colors("rgbk") == [tuple(c) for c in DEFAULT_PALETTE] == parse_pen_colors(" RGBK ")
    assert parse_pen_colors("#f00, blue,#00ff00") == [(255, 0, 0), (0, 0, 255), (0, 255, 0)]
    assert len(parse_pen_colors(",".join(["red"] * 8))) == 8
    for bad in ("", "red,,blue", "nocolor", ",".join(["red"] * 9), "rgb(1,2,3)", "none"):
        with pytest.raises(ValueError):
            parse_pen_colors(bad)


def test_nearest_pen_and_ties():
    from orip.svg import nearest_pen
    pal = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0)]
    rgb = [(250, 10, 10), (0, 128, 0), (120, 120, 120), (127, 0, 0), (128, 0, 0), (-1, -1, -1), (255, 255, 255), (0, 0, 127)]
    # (0, 128, 0): 127^2 from green, 128^2 from black; grey (120, 120, 120): 43200 from black, 47025 from each of the others; (127, 0, 0) is nearer black, (128, 0, 0) nearer red;
    # white: 2 * 255^2 from each of R, G, B -> the lowest index; (0, 0, 127): black by 127^2 against 128^2
    assert nearest_pen(rgb, pal).tolist() == [0, 1, 3, 3, 0, -1, 0, 3]
    assert nearest_pen([(10, 10, 10)], [(0, 0, 0), (20, 20, 20), (0, 0, 0)]).tolist() == [0]         # an exact tie, and a repeated entry: the lowest index
    assert nearest_pen(np.zeros((0, 3)), pal).tolist() == []


def test_stroke_and_fill_are_parsed_and_inherited():
    from orip.svg import parse_svg
    t = parse_svg(svg('<g stroke="red" fill="#00f"><path d="M0 0 L5 5 M6 6 L7 7"/><g style="stroke:lime"><line x1="0" y1="0" x2="3" y2="3"/>'
                      '<rect width="4" height="4" stroke="none" style="fill: rgb(10,20,30); stroke-width:3"/></g>'
                      '<circle r="3" style="stroke-width: 2" fill="url(#p)"/></g><polyline points="0,0 1,1" stroke="currentColor"/><path d="M1 1 L2 2"/>'))
    assert t.n_sub == 7 and t.stroke_rgb.dtype == np.int16 and t.fill_rgb.dtype == np.int16 and t.stroke_rgb.shape == t.fill_rgb.shape == (7, 3)
    R, L, N = [255, 0, 0], [0, 255, 0], [-1, -1, -1]
    assert t.stroke_rgb.tolist() == [R, R, L, N, R, N, N]                 # both subpaths of the path; the style property beats the group; none; stroke-width is not stroke
    assert t.fill_rgb.tolist() == [[0, 0, 255]] * 3 + [[10, 20, 30], N, N, N]
    assert t.fill_group.tolist() == [0, 0, -1, 2, 3, -1, -1]              # as before: a line is never hatched, url(...) is a stated fill
    from orip.svg import SegmentTable
    old = SegmentTable(t.kind, t.ctrl, t.mat, t.sub_off, t.closed, t.mats)                           # existing constructions keep working
    assert old.stroke_rgb is None and old.fill_rgb is None and old.fill_group is None


def test_pens_of_paths_and_hatch_lines():
    from orip.svg import parse_svg, subpath_pens, hatch_pens, parse_pen_colors
    pal = parse_pen_colors("rgbk")
    t = parse_svg(svg('<rect width="9" height="9" fill="#0e0" stroke="#f00"/><path d="M0 0 L1 1"/><circle r="4" stroke="blue"/><circle r="2" fill="#111"/>'), "all")
    assert subpath_pens(t, pal).tolist() == [0, -1, 2, -1]
    assert t.fill_group.tolist() == [0, 1, 2, 3]
    # the fill colour where there is one, else the stroke (--hatch-fill all), else nothing
    assert hatch_pens(t, [0, 0, 2, 3, 1, 0], pal).tolist() == [1, 1, 2, 3, -1, 1] and hatch_pens(t, [], pal).tolist() == []
    with pytest.raises(RuntimeError):
        hatch_pens(t, [4], pal)


# ------------------------------------------------------------------ T words
def test_t_words_in_parse_gcode():
    from orip.gcode import parse_gcode
    text = "G21 G90\nG0 X1 Y1\nM3\nG1 X2 Y2\nM5\nT2\nG0 X5 Y5\nM3\nT1 G1 X6 Y6\nG1 X7 Y7\nM5\nt3 (a comment) M3\nG1 X8 Y8\nM5 T0\nG0 X0 Y0\nM3 G1 X1 Y0\nTx\nM5\n"
    a = parse_gcode(text)
    pens = []
    b = parse_gcode(text, pens)
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and a[2] == b[2] and len(a) == 3     # the return value is what it was
    # no T yet; the T of the line of the first pen-down move counts, a later one does not change the open path; lower case; T0; a word without a number
    assert pens == [-1, 1, 3, 0]
    for bad in ("T8\nM3 G1 X1 Y1\n", "T-1\nM3 G1 X1\n", "T255"):
        parse_gcode(bad)                                                  # skipped, as ever
        with pytest.raises(ValueError):
            parse_gcode(bad, [])


def test_gcode_text_round_trips_the_pens():
    from orip.svg import gcode_text
    from orip.gcode import parse_gcode
    off = np.array([0, 2, 4, 7, 9, 11]); pts = np.arange(22).reshape(11, 2) * 0.5
    plain = gcode_text(off, pts)
    assert "T" not in plain and gcode_text(off, pts, pens=None) == plain
    text = gcode_text(off, pts, pens=[3, 3, 0, 7, 7])
    assert [ln for ln in text.splitlines() if ln.startswith("T")] == ["T3", "T0", "T7"]
    assert [ln for ln in text.splitlines() if not ln.startswith("T")] == plain.splitlines()
    pens = []
    o2, p2, _ = parse_gcode(text, pens)
    assert pens == [3, 3, 0, 7, 7] and np.array_equal(o2, off) and np.array_equal(p2, pts)
    assert all(np.array_equal(a, b) for a, b in zip(parse_gcode(text)[:2], parse_gcode(plain)[:2]))
    with pytest.raises(ValueError):
        gcode_text(off, pts, pens=[1, 2])


def test_pen_sequence():
    from orip.gcode import pen_sequence
    assert pen_sequence(None) == list(range(8)) == pen_sequence("")
    assert pen_sequence("3, 0") == [3, 0, 1, 2, 4, 5, 6, 7]
    for bad in ("8", "1,1", "x", "-1"):
        with pytest.raises(ValueError):
            pen_sequence(bad)


# ------------------------------------------------------------------ command lines
def test_cli_defaults():
    from orip import svg as SV, gcode as GC
    a = SV.build_stream_argparser().parse_args(["in.svg"])
    assert a.pen_colors is None and a.pen_order is None and a.allow_reverse is False
    o = SV.options_from_args(a)
    assert o.pen_colors is None and o.pen_order is None and o.allow_reverse is False
    go = SV.gcode_options(o)
    assert go.allow_reverse is False and go.tool_pens is False and go.pen_order is None
    g = SV.build_gcode_argparser().parse_args(["in.svg"])
    assert g.pen_colors is None and not hasattr(g, "allow_reverse")
    c = GC.build_argparser().parse_args(["in.gcode"])
    assert c.allow_reverse is False and c.tool_pens is False and c.pen_order is None
    o = stream_options(["--pen-colors", "rgbk", "--pen-order", "3,0", "--allow-reverse"])
    go = SV.gcode_options(o)
    assert (o.pen_colors, go.pen_order, go.allow_reverse) == ("rgbk", "3,0", True)
    assert GC.options_from_args(GC.build_argparser().parse_args(["in.gcode", "--tool-pens", "--allow-reverse", "--pen-order", "2"])).tool_pens is True
    with pytest.raises(ValueError):
        SV.build_stream_from_svg(svg('<path d="M0 0 L1 1"/>'), stream_options(["--pen-colors", "nocolor"]), **PD.pens_doubles())


# ------------------------------------------------------------------ nothing changes without the options
def never(*a, **k):
    raise AssertionError("a device step of the pens was called without a pen option")


def test_gcode_bytes_unchanged_without_the_options():
    from orip.gcode import build_stream_from_gcode
    from test_gcode_host import G, MAIN_CASES, options_for, DOUBLES
    for i, (name, args) in enumerate(MAIN_CASES):
        data, info = build_stream_from_gcode(bytes(G[f"text_{name}"]), options_for(args), order_pens_fn=never, source_fn=never, **DOUBLES)
        assert data == bytes(G[f"main_{i}_bin"]) and "pens" not in info


def test_svg_bytes_unchanged_without_the_options():
    from orip import svg as SV
    from test_svg_host import G, ARGS, RUNS, options_for
    for i, (name, key) in enumerate(RUNS):
        data, info = SV.build_stream_from_svg(bytes(G[f"svg_{name}"]), options_for(ARGS[key]), order_pens_fn=never, source_fn=never, hatch_groups_fn=never, **SD.svg_doubles())
        assert data == bytes(G[f"run_{i}_bin"]) and "pens" not in info and "path_pens" not in info
    data, info = SV.build_stream_from_svg(PD.TOOL_SVG, stream_options(PD.TOOL_PLAIN_ARGS), order_pens_fn=never, source_fn=never, hatch_groups_fn=never,
                                          **dict(SD.svg_doubles(), hatch_fn=HD.hatch_numpy))
    assert data == bytes(GP["tool_plain_stream"])


# ------------------------------------------------------------------ the whole host path with pens, through the doubles
def split_stream(data):
    """service bytes of a stream up to its end byte, step bytes left out"""
    out = []
    for b in data:
        if b == 0x3F:
            break
        if b < 0x40:
            out.append(b)
    return out


def test_tool_svg_through_the_doubles():
    from orip import svg as SV
    data, info = SV.build_stream_from_svg(PD.TOOL_SVG, stream_options(PD.TOOL_PEN_ARGS), want_paths=True, **PD.pens_doubles())
    n_sub, seg = info["subpaths"], info["hatch"]["segments"]
    assert n_sub == 7 and seg > 10 and info["paths"] == n_sub + seg
    assert info["path_pens"].tolist() == [0, 0, 1, 2, 2, 3, 1] + [3] * seg                          # the rectangle states no stroke: --color-index, 3
    assert info["pens"] == {"paths": [2, 2, 2, 1 + seg, 0, 0, 0, 0], "unmatched": 1, "reversed": info["pens"]["reversed"]} and info["pens"]["reversed"] > 0
    svc = split_stream(data)
    assert svc[0] == 0x01 and [b & 7 for b in svc if 0x08 <= b <= 0x0F] == [0, 1, 2, 3]               # one colour byte per pen, ascending
    assert svc.count(0x02) == info["paths"]
    # another pen for what states no stroke, another drawing order, and file order inside a pen
    d2, i2 = SV.build_stream_from_svg(PD.TOOL_SVG, stream_options(PD.TOOL_PEN_ARGS + ["--color-index", "5", "--pen-order", "3,5,0"]), **PD.pens_doubles())
    assert [b & 7 for b in split_stream(d2) if 0x08 <= b <= 0x0F] == [3, 5, 0, 1, 2] and i2["pens"]["paths"] == [2, 2, 2, seg, 0, 1, 0, 0]
    d3, i3 = SV.build_stream_from_svg(PD.TOOL_SVG, stream_options(PD.TOOL_PLAIN_ARGS + ["--pen-colors", "rgbk", "--no-reorder"]), **dict(PD.pens_doubles(), order_pens_fn=never))
    assert [b & 7 for b in split_stream(d3) if 0x08 <= b <= 0x0F] == [0, 1, 2, 3] and i3["pens"]["reversed"] == 0
    # the G-code names the pens, and gcode2stream --tool-pens draws the same stream from it
    from orip import gcode as GC
    text = SV.gcode_text(*info["fitted_paths"], pens=info["path_pens"])
    S = PD.StepsWithSource()
    again, ginfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(tool_pens=True, allow_reverse=True), steps_fn=S.steps, source_fn=S.source, order_fn=never,
                                              order_pens_fn=PD.order_pens_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)
    assert again == data and ginfo["pens"]["unmatched"] == 0 and ginfo["pens"]["paths"] == info["pens"]["paths"]


def test_allow_reverse_alone_keeps_the_head():
    from orip import gcode as GC
    from test_gcode_host import G, DOUBLES
    text = bytes(G["text_drawing"])
    S = PD.StepsWithSource()
    dbl = dict(DOUBLES, steps_fn=S.steps, source_fn=S.source, order_pens_fn=PD.order_pens_numpy)
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(), **DOUBLES)
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(allow_reverse=True), **dbl)
    assert "pens" not in info and info["reversed"] > 0 and info["paths"] == pinfo["paths"]
    assert split_stream(data)[:2] == split_stream(plain)[:2] == [0x01, 0x08 | 3] and data[:3] == plain[:3]        # [pen up, speed, colour]
    assert split_stream(data).count(0x02) == info["paths"] and data != plain
