"""The dash pass on the host, without a GPU: on the named drawings of tests/dash_cases.py and on seeded random ones the sequential double
(tests/dash_double.py) keeps every consequence include/orip.h draws from the rule; the parser records stroke-dasharray and stroke-dashoffset as it records
the stroke; the patterns are scaled as stated; both command lines and every argument error; and the host flow of both tools with every device step injected
as a double: the pass sits behind the pens and in front of the occlusion and the dedup, pens follow origin, without the options nothing is called and every
byte is what it was, and a return that does not hold is refused.  No comparison here has a tolerance."""
from fractions import Fraction

import numpy as np
import pytest

import dash_cases as DC
import dash_double as DD
import gcode_double as D
import pens_double as PD
from stream_double import codes_numpy

CASES = DC.cases()
U = 256
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)


def never(*a, **k):
    raise AssertionError("the dash pass was called without its option")


class Recorder:
    """a double that remembers what it was given and what it returned, and writes its name into a shared log"""
    def __init__(self, fn, name="dash", log=None): self.fn, self.name, self.calls, self.log = fn, name, [], log if log is not None else []

    def __call__(self, *a):
        out = self.fn(*a)
        self.calls.append((a, out)); self.log.append(self.name)
        return out


def gcode_steps():
    S = PD.StepsWithSource()
    return dict(GCODE_DOUBLES, steps_fn=S.steps, source_fn=S.source)


# ------------------------------------------------------------------ the rule, on the double
def strokes_of(off, pts):
    return [[tuple(q) for q in pts[a:b].tolist()] for a, b in zip(off[:-1], off[1:])]


def exact_point(v, S, s):
    """the exact rational point of the stroke at arc position s"""
    j = max(k for k in range(len(S)) if S[k] <= s)
    if S[j] == s:
        return tuple(Fraction(c) for c in v[j])
    return tuple(Fraction(a) + Fraction(s - S[j], S[j + 1] - S[j]) * (b - a) for a, b in zip(v[j], v[j + 1]))


def consequences(case):
    off, pts, pattern, phase, po, pv = case
    out_off, out_pts, origin, st = DD.dash_numpy(*case)
    ins, outs = strokes_of(off, pts), strokes_of(out_off, out_pts)
    assert st["paths_out"] == st["paths_in"] - st["dashed"] + st["dashes"] - st["collapsed"] == len(outs) and st["points_out"] == len(out_pts)
    assert 0 <= st["length_on"] <= st["length_in"] and st["dashed"] == int((pattern >= 0).sum())
    assert (np.diff(origin) >= 0).all()
    for k, d in zip(origin.tolist(), outs):
        v = ins[k]
        assert len(d) >= 2 and all(a != b for a, b in zip(d[:-1], d[1:]))
        if pattern[k] < 0:
            assert d == v
            continue
        inner = d[1:-1]                                                            # input vertices, in order
        at = [j for j in range(len(v)) if v[j] == inner[0]] if inner else [0]
        assert any(v[j:j + len(inner)] == inner for j in at)
    if not len(origin) or len(pts) > 5000:
        return
    for k in range(len(ins)):                                                      # the two ends of every dash lie within half a step of the exact point
        if pattern[k] < 0:
            assert sum(1 for q in origin if q == k) == 1
            continue
        pat = pv[po[pattern[k]]:po[pattern[k] + 1]].tolist()
        dashes, _, _ = DD.dash_stroke(ins[k], pat, int(phase[k]))
        S = DD.lengths(ins[k])
        P, A = sum(pat), np.concatenate([[0], np.cumsum(pat)]).tolist()
        spans = []
        r = 0
        while r * P - int(phase[k]) < S[-1]:
            for i in range(0, len(pat), 2):
                s0, s1 = max(r * P + A[i] - int(phase[k]), 0), min(r * P + A[i + 1] - int(phase[k]), S[-1])
                if s1 > s0:
                    spans.append((s0, s1))
            r += 1
        assert len(spans) == len(dashes)
        for (s0, s1), d in zip(spans, dashes):
            for s, got in ((s0, d[0]), (s1, d[-1])):
                want = exact_point(ins[k], S, s)
                assert all(abs(Fraction(g) - w) <= Fraction(1, 2) for g, w in zip(got, want))


@pytest.mark.parametrize("name", sorted(CASES))
def test_consequences_on_the_named_drawings(name):
    consequences(CASES[name])


def test_the_named_drawings_do_what_their_names_say():
    st = {k: DD.dash_numpy(*v)[3] for k, v in CASES.items()}
    assert st["a_thousand_dashes"]["dashes"] >= 2 * 980                           # 3700 steps and more, 3.75 to the period, twice
    assert st["everything_vanishes"]["paths_out"] == 0 and st["wholly_in_a_gap"]["paths_out"] == 1
    assert st["one_step_dashes_on_diagonals"]["collapsed"] > 0 and st["axis_parallel_whole_steps"]["collapsed"] == 0
    assert st["dash_longer_than_the_stroke"]["dashes"] == 2 and st["seventy_thousand_points"]["points_out"] > 50000
    per_stroke = np.bincount(DD.dash_numpy(*CASES["two_points_every_count"])[2])
    assert set(range(1, 25)) <= set(per_stroke.tolist())                          # every number of dashes from 1 up, on both sides of the hand-over to a wave
    off, pts, pattern, phase, po, pv = CASES["two_points_every_count"]
    cuts = {DC.cut_points(int(x1 - x0) * U, pv.tolist(), 0) for (x0, _), (x1, _) in pts.reshape(-1, 2, 2).tolist()}
    assert set(range(20, 30)) <= cuts                                             # and every number of cut points around the hand-over itself
    off, pts, pattern, phase, po, pv = CASES["two_points_around_the_wave_stride"]
    per_stroke = np.bincount(DD.dash_numpy(off, pts, pattern, phase, po, pv)[2])
    assert {63, 64, 65} <= set(per_stroke.tolist())                               # the wave's stride: 63, 64 and 65 dashes,
    cuts = {DC.cut_points(abs(int(x1 - x0)) * U, pv.tolist(), int(h)) for ((x0, _), (x1, _)), h in zip(pts.reshape(-1, 2, 2).tolist(), phase)}
    assert {63, 64, 65} | set(range(126, 131)) <= cuts                            # and 63, 64, 65 and 126 .. 130 cut points


def test_consequences_on_random_drawings():
    for seed in range(300):
        consequences(DC.random_drawing(seed))


def test_a_whole_number_of_periods_is_on_in_proportion():
    pat = [3 * U, 2 * U, U, 4 * U]                                                # P = 10 steps, 4 of them on
    for n_periods in (1, 2, 7):
        st = DD.dash_numpy(*DC.drawing([[(5, 5), (5 + 10 * n_periods, 5)]], [0], [0], [pat]))[3]
        assert st["length_in"] == 10 * n_periods * U and st["length_on"] * sum(pat) == st["length_in"] * (pat[0] + pat[2])
    case = DC.drawing([[(0, 0), (30, 40), (30, 90)]], [0], [0], [pat])           # 50 + 50 steps, exact square roots
    st = DD.dash_numpy(*case)[3]
    assert st["length_in"] == 100 * U and st["length_on"] == 40 * U


def test_a_first_dash_as_long_as_the_stroke_returns_it_unchanged():
    for lists in ([[(3, 3), (9, 7), (4, 12)]], [[(0, 0), (13, 0)]]):
        S_end = DD.lengths(lists[0])[-1]
        for first in (S_end, S_end + 1, 1 << 40):
            off, pts, origin, st = DD.dash_numpy(*DC.drawing(lists, [0], [0], [[max(first, U), U]]))
            assert strokes_of(off, pts) == lists and origin.tolist() == [0] and st["dashes"] == 1 and st["length_on"] == st["length_in"] == S_end
    off, pts, origin, st = DD.dash_numpy(*DC.drawing([[(0, 0), (13, 0)]], [0], [0], [[13 * U - 1, U]]))       # one unit short: the end is cut off
    assert strokes_of(off, pts) == [[(0, 0), (13, 0)]] and st["length_on"] == 13 * U - 1      # and rounds back onto the vertex


def test_a_drawing_without_a_dashed_stroke_comes_back_unchanged():
    off, pts, pattern, phase, po, pv = CASES["mixed_patterns"]
    out = DD.dash_numpy(off, pts, np.full(len(pattern), -1), phase * 0, po, pv)
    assert np.array_equal(out[0], off) and np.array_equal(out[1], pts) and out[2].tolist() == list(range(len(off) - 1))
    assert out[3]["dashed"] == out[3]["dashes"] == out[3]["length_in"] == 0


def lattice_steps(strokes):
    """the primitive lattice steps of axis-parallel strokes, in order, as (doubled midpoint x, doubled midpoint y)"""
    out = []
    for s in strokes:
        for (x0, y0), (x1, y1) in zip(s[:-1], s[1:]):
            n = max(abs(x1 - x0), abs(y1 - y0)); dx, dy = (x1 - x0) // n, (y1 - y0) // n
            assert (dx == 0) != (dy == 0)
            out += [(2 * (x0 + i * dx) + dx, 2 * (y0 + i * dy) + dy) for i in range(n)]
    return out


def test_axis_parallel_strokes_with_whole_step_patterns_keep_exactly_the_steps_whose_midpoint_is_on():
    cases = [CASES["axis_parallel_whole_steps"]]
    rng = np.random.default_rng(3)
    for _ in range(60):
        lists = []
        for _ in range(3):
            v = [(int(rng.integers(0, 30)), int(rng.integers(0, 30)))]
            for _ in range(int(rng.integers(1, 6))):
                d = int(rng.integers(1, 15))
                q = (v[-1][0] + d, v[-1][1]) if rng.random() < 0.5 else (v[-1][0], v[-1][1] + d * (1 if rng.random() < 0.5 or v[-1][1] < d else -1))
                v.append(q)
            lists.append(v)
        pat = [U * int(rng.integers(1, 6)) for _ in range(int(rng.choice([2, 4, 6])))]
        cases.append(DC.drawing(lists, [0] * 3, [U * int(rng.integers(0, sum(pat) // U)) for _ in range(3)], [pat]))
    for case in cases:
        off, pts, pattern, phase, po, pv = case
        out_off, out_pts, origin, st = DD.dash_numpy(*case)
        assert st["collapsed"] == 0
        outs = strokes_of(out_off, out_pts)
        for k, v in enumerate(strokes_of(off, pts)):
            pat = pv[po[pattern[k]]:po[pattern[k] + 1]].tolist()
            P, A = sum(pat), np.concatenate([[0], np.cumsum(pat)]).tolist()
            on = lambda s2: any(A[i] <= (s2 * (U // 2) + int(phase[k])) % P < A[i + 1] for i in range(0, len(pat), 2))      # s2: doubled arc position in steps
            want = [m for i, m in enumerate(lattice_steps([v])) if on(2 * i + 1)]
            assert lattice_steps([d for q, d in zip(origin.tolist(), outs) if q == k]) == want


def test_nothing_depends_on_the_order_of_the_strokes_or_on_their_neighbours():
    off, pts, pattern, phase, po, pv = CASES["mixed_patterns"]
    whole = DD.dash_numpy(off, pts, pattern, phase, po, pv)
    outs = strokes_of(whole[0], whole[1])
    for k in range(len(off) - 1):
        alone = DD.dash_numpy(np.array([0, off[k + 1] - off[k]]), pts[off[k]:off[k + 1]], pattern[k:k + 1], phase[k:k + 1], po, pv)
        assert strokes_of(alone[0], alone[1]) == [d for q, d in zip(whole[2].tolist(), outs) if q == k]


def test_the_double_refuses_what_the_device_refuses():
    o, p = np.array([0, 2]), np.array([[0, 0], [9, 0]])
    good = ([0], [0], [0, 2], [512, 256])
    DD.dash_numpy(o, p, *good)
    for bad in (([1], [0], [0, 2], [512, 256]), ([-2], [0], [0, 2], [512, 256]), ([0], [768], [0, 2], [512, 256]), ([0], [-1], [0, 2], [512, 256]), ([0], [0], [0, 1], [512, 256]),
                ([0], [0], [0, 3], [512, 256, 300]), ([0], [0], [0, 0], []), ([0], [0], [0, 66], [300] * 66), ([0], [0], [0, 2], [512, 255]), ([0], [0], [0, 2], [512, (1 << 40) + 1]),
                ([0], [0], [1, 2], [512, 256]), ([0, 0], [0], [0, 2], [512, 256])):
        with pytest.raises(ValueError):
            DD.dash_numpy(o, p, *bad)
    with pytest.raises(ValueError):
        DD.dash_numpy(o, np.array([[0, 0], [0, 0]]), *good)


# ------------------------------------------------------------------ the parser
SVG = b"""<svg xmlns="http://www.w3.org/2000/svg" width="100" height="100" viewBox="0 0 100 100">
 <g stroke="black" stroke-dasharray="4 2" stroke-dashoffset="1">
  <line id="inherits" x1="0" y1="0" x2="50" y2="0"/>
  <line id="own attribute" x1="0" y1="5" x2="50" y2="5" stroke-dasharray="3,1,2"/>
  <line id="style over attribute" x1="0" y1="10" x2="50" y2="10" stroke-dasharray="9 9" style="stroke:red;stroke-dasharray: 5px 2.5px ; stroke-dashoffset:-3"/>
  <g style="stroke-dasharray:none"><line id="none through a group" x1="0" y1="15" x2="50" y2="15"/><path id="two subpaths" stroke-dasharray="1 1" d="M0 20 L50 20 M0 25 L50 25"/></g>
 </g>
 <line id="nobody says" x1="0" y1="30" x2="50" y2="30" stroke="black"/>
</svg>"""


def test_the_parser_records_dash_array_and_offset_of_every_subpath():
    from orip import svg as SV
    t = SV.parse_svg(SVG)
    assert t.dash_array == ["4 2", "3,1,2", "5px 2.5px", "none", "1 1", "1 1", None] and t.dash_offset == ["1", "1", "-3", "1", "1", "1", None]
    assert len(t.dash_array) == t.n_sub == 7
    f = SV.SegmentTable.__dataclass_fields__
    assert list(f)[-2:] == ["dash_array", "dash_offset"] and f["dash_array"].default is None and f["dash_offset"].default is None
    assert SV.SegmentTable(*[None] * 6).dash_array is None


def test_what_a_dash_array_says():
    from orip import svg as SV
    P = SV.parse_dasharray
    assert P("4 2") == [4.0, 2.0] and P("3,1,2") == [3.0, 1.0, 2.0] and P(" 5px , 2.5mm ") == [5.0, 2.5] and P("1e1 .5") == [10.0, 0.5] and P("0 0") == [0.0, 0.0]
    for solid in (None, "none", "NONE", "", "4 -2", "50% 2", "4 two", "4;2", "inherit", "nan 2", "inf"):
        assert P(solid) is None, solid


def test_the_patterns_are_scaled_per_subpath_and_shared():
    from orip import svg as SV
    text = b"""<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 100 100"><g stroke="black">
     <line x1="0" y1="0" x2="50" y2="0" stroke-dasharray="4 2" stroke-dashoffset="1"/>
     <g transform="scale(2)"><line x1="0" y1="5" x2="25" y2="5" stroke-dasharray="2 1" stroke-dashoffset="-1"/></g>
     <g transform="matrix(4 0 0 1 0 0)"><line x1="0" y1="10" x2="10" y2="10" stroke-dasharray="3"/></g>
     <line x1="0" y1="20" x2="50" y2="20" stroke-dasharray="0 0"/><line x1="0" y1="21" x2="50" y2="21" stroke-dasharray="4 0.001"/>
     <line x1="0" y1="22" x2="50" y2="22" stroke-dasharray="1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 19 20 21 22 23 24 25 26 27 28 29 30 31 32 33"/>
     <line x1="0" y1="23" x2="50" y2="23" stroke-dasharray="4 -2"/><line x1="0" y1="24" x2="50" y2="24"/></g></svg>"""
    t = SV.parse_svg(text)
    pattern, phase, po, pv, ignored = SV.dash_patterns(t, (1.5, 1.5, 0.0, 0.0), 40.0, t.n_sub + 2)        # two hatch lines behind the subpaths
    k = 1.5 * 40.0 * 256
    assert pattern.tolist() == [0, 0, 1, -1, -1, -1, -1, -1, -1, -1] and ignored == 3                   # zero sum, under a step, 66 entries; the negative is just solid
    assert po.tolist() == [0, 2, 4] and pv.tolist() == [int(round(4 * k)), int(round(2 * k)), int(round(3 * 2 * k)), int(round(3 * 2 * k))]      # sqrt(4 x 1) = 2; 3 doubled to 3 3
    P = int(pv[:2].sum())
    assert phase.tolist()[:3] == [int(round(1 * k)), int(round(-1 * 2 * k)) % P, 0] and 0 <= phase[1] < P
    assert pattern.dtype == np.int32 and phase.dtype == np.int64 and po.dtype == np.int32 and pv.dtype == np.int64
    sx_sy = SV.dash_patterns(t, (4.0, 1.0, 0.0, 0.0), 40.0, t.n_sub)[3]                                 # a non-uniform fit: the mean scale
    assert sx_sy[0] == int(round(4 * 2.0 * 40.0 * 256))
    plain = SV.parse_svg(PD.TOOL_SVG)
    assert SV.dash_patterns(plain, (1.0, 1.0, 0, 0), 40.0, plain.n_sub)[0].tolist() == [-1] * plain.n_sub
    assert SV.dash_patterns(SV.SegmentTable(*[plain.kind, plain.ctrl, plain.mat, plain.sub_off, plain.closed, plain.mats]), (1.0, 1.0, 0, 0), 40.0, 3)[0].tolist() == [-1] * 3


# ------------------------------------------------------------------ the command lines
def gcode_options(args):
    from orip import gcode as GC
    return GC.options_from_args(GC.build_argparser().parse_args(["in.gcode"] + list(args)))


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def test_options_parse_on_both_tools_and_the_pinned_records_stand():
    from orip import svg as SV, gcode as GC
    assert GC.GcodeOptions().dash_mm is None and GC.GcodeOptions().dash_offset_mm is None and SV.SvgOptions().dashes is False
    assert [f for f in GC.GcodeOptions.__dataclass_fields__][-2:] == ["dash_mm", "dash_offset_mm"] and list(SV.SvgOptions.__dataclass_fields__)[-1] == "dashes"
    o = gcode_options(["--dash-mm", "2,1", "--dash-offset-mm", "-0.5"])
    assert (o.dash_mm, o.dash_offset_mm) == ("2,1", -0.5) and GC.dash_option(o) == ([2 * 40 * U, 40 * U], (-20 * U) % (120 * U))
    assert GC.dash_option(gcode_options(["--dash-mm", "1.5"])) == ([60 * U, 60 * U], 0)                 # an odd count is doubled, as SVG does
    assert GC.dash_option(gcode_options(["--dash-mm", "1,2,3", "--dash-offset-mm", "100"])) == ([40 * U, 80 * U, 120 * U] * 2, (4000 * U) % (480 * U))
    assert GC.dash_option(gcode_options([])) is None
    assert GC.dash_option(gcode_options(["--dash-mm", "0.025", "--steps-per-mm", "40"]))[0] == [U, U]  # exactly one step
    assert svg_options(["--dashes"]).dashes is True and svg_options([]).dashes is False
    assert not hasattr(SV.build_gcode_argparser().parse_args(["in.svg"]), "dashes")                     # svg2gcode.py writes G-code: the pass lives in the stream
    assert SV.gcode_options(svg_options(["--dashes"])).dash_mm is None                                  # the SVG door brings its own record
    import recording_device as RD
    gcode_steps, svg_steps = RD.doors_take_the_pass_table()
    assert GC.STROKE_ARGS[-1] == "--dedup" and len(GC.STROKE_ARGS) == 10 and "dash_fn" in gcode_steps and "dash_fn" in svg_steps
    assert [p.name for p in GC.PASSES].index("dash") == [p.name for p in GC.PASSES].index("convert") + 1
    assert "--dash-mm" not in GC.STROKE_ARGS and GC.DASH_STATS == DD.DASH_STATS


@pytest.mark.parametrize("args,word", [(["--dash-mm", "0.02"], "0.800781 steps"), (["--dash-mm", "2,-1"], "-1"), (["--dash-mm", "2,x"], "'2,x'"), (["--dash-mm", ""], "''"),
                                       (["--dash-mm", ",".join(["1"] * 65)], "65 lengths"), (["--dash-mm", ",".join(["1"] * 33)], "66 entries"),
                                       (["--dash-mm", "2,nan"], "nan"), (["--dash-mm", "2,inf"], "inf"), (["--dash-mm", "2,0"], "0 steps"),
                                       (["--dash-mm", "1e9", "--steps-per-mm", "40"], "steps"), (["--dash-offset-mm", "1"], "needs --dash-mm"),
                                       (["--dash-mm", "2,1", "--dash-offset-mm", "nan"], "--dash-offset-mm")])
def test_argument_errors_name_the_value(args, word, tmp_path):
    from orip import gcode as GC
    with pytest.raises(ValueError) as e:
        GC.dash_option(gcode_options(args))
    assert word in str(e.value)
    (tmp_path / "in.gcode").write_text(DC.TOOL_GCODE)
    with pytest.raises(ValueError):                                               # and the tool ends before any device step
        GC.main([str(tmp_path / "in.gcode"), "-o", str(tmp_path / "out.bin")] + args, dash_fn=never, steps_fn=never, order_fn=never, codes_fn=never, pack_fn=never)


# ------------------------------------------------------------------ the host flow through the doubles
def test_off_by_default_and_bytes_unchanged():
    from orip import gcode as GC, svg as SV
    from test_gcode_host import G, MAIN_CASES, options_for
    for i, (name, args) in enumerate(MAIN_CASES):                                 # the streams written down before this pass existed
        data, info = GC.build_stream_from_gcode(bytes(G[f"text_{name}"]), options_for(args), dash_fn=never, **GCODE_DOUBLES)
        assert data == bytes(G[f"main_{i}_bin"]) and "dash" not in info
    o = svg_options(["--pen-colors", "#f00,#00f"])
    a = SV.build_stream_from_svg(DC.TOOL_SVG, o, **PD.pens_doubles())
    b = SV.build_stream_from_svg(DC.TOOL_SVG, o, dash_fn=never, **PD.pens_doubles())
    assert a[0] == b[0] and "dash" not in b[1]
    c = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(["--dashes", "--pen-colors", "#f00,#00f"]), dash_fn=never, **PD.pens_doubles())      # no dash array stated: no call
    d = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(["--pen-colors", "#f00,#00f"]), **PD.pens_doubles())
    assert c[0] == d[0] and "dash" not in c[1]
    only_ignored = DC.TOOL_SVG.replace(b"4 2", b"0 0").replace(b"1.5, 3, 5", b"0.0001 3").replace(b'stroke-dashoffset="-1"', b"")
    e = SV.build_stream_from_svg(only_ignored, svg_options(["--dashes"]), dash_fn=never, **PD.pens_doubles())       # every array ignored: no call either
    f = SV.build_stream_from_svg(only_ignored, svg_options([]), **PD.pens_doubles())
    assert e[0] == f[0] and e[1]["dash"] == {"ignored": 3}                        # and the report says that three strokes stay solid
    from orip import gcode as GC
    assert list(GC.report_lines("svg", e[1]))[-1].startswith("[svg] dash: no stroke dashed, 3 dash arrays ignored")


def test_gcode_flow_dashes_every_path_and_pens_follow_origin():
    from orip import gcode as GC
    import merge_cases as MC
    lines = ["G21 G90 M5"]
    paths = [(1, [(10, 10), (30, 10)]), (2, [(10, 20), (30, 20), (30, 35)]), (1, [(50, 50), (50.01, 50)]), (5, [(5, 60), (45.5, 71.3)])]
    for t, s in paths:
        lines += ["T%d" % t, "G0 X%g Y%g" % s[0], "M3"] + ["G1 X%g Y%g" % q for q in s[1:]] + ["M5"]
    text = "\n".join(lines) + "\n"
    Z, tm = Recorder(DD.dash_numpy), {}
    o = gcode_options(["--dash-mm", "3,1.5", "--dash-offset-mm", "1", "--tool-pens"])
    data, info = GC.build_stream_from_gcode(text, o, dash_fn=Z, order_pens_fn=PD.order_pens_numpy, timings=tm, **gcode_steps())
    (off, pts, pattern, phase, po, pv), out = Z.calls[0]
    assert len(Z.calls) == 1 and "dash" in tm and len(off) - 1 == 3                # the path of a quarter step is dropped by the conversion
    assert pattern.tolist() == [0, 0, 0] and phase.tolist() == [40 * U] * 3 and po.tolist() == [0, 2] and pv.tolist() == [120 * U, 60 * U]
    assert info["dash"] == out[3] and info["paths"] == out[3]["paths_out"] == len(out[2]) > 10
    pen_of = np.array([1, 2, 5])[out[2]]                                          # a dash is drawn with its stroke's pen
    drawn = MC.strokes_of(data)
    assert sorted((c, s[0], s[-1]) for c, s in drawn) == sorted((int(c), tuple(out[1][a]), tuple(out[1][b - 1])) for c, a, b in zip(pen_of, out[0][:-1], out[0][1:]))
    assert info["pens"]["paths"][1] + info["pens"]["paths"][2] + info["pens"]["paths"][5] == 3
    line = list(GC.report_lines("gcode", info))[-1]
    assert line.startswith("[gcode] dash: 3 strokes dashed, ") and line.endswith(f"-> {info['paths']} strokes")
    plain, pinfo = GC.build_stream_from_gcode(text, gcode_options(["--tool-pens"]), dash_fn=never, order_pens_fn=PD.order_pens_numpy, **gcode_steps())
    assert pinfo["paths"] == 3 and "dash" not in pinfo


def test_the_pass_sits_behind_the_pens_and_in_front_of_the_occlusion_and_the_dedup():
    from orip import svg as SV
    import dedup_double as DDD
    import clip_double as CD
    import occlude_cases as OC
    log = []
    Z = Recorder(DD.dash_numpy, "dash", log)
    dbl = CD.svg_doubles()
    dbl = dict(dbl, source_fn=Recorder(dbl["source_fn"], "source", log), dash_fn=Z, dedup_fn=Recorder(DDD.dedup_numpy, "dedup", log),
               occlude_fn=Recorder(OC.OccludeDouble(), "occlude", log))
    text = DC.TOOL_SVG.replace(b'<rect x="5" y="5" width="90" height="70" stroke="black" fill="none"/>', b'<rect x="40" y="5" width="20" height="70" stroke="black" fill="white"/>')
    data, info = SV.build_stream_from_svg(text, svg_options(["--dashes", "--occlude", "--dedup", "--pen-colors", "#000,#f00"]), **dbl)
    assert [w for w in log if w != "source"] == ["dash", "occlude", "dedup"] and log[0] == "source"
    (off, pts, pattern, phase, po, pv), out = Z.calls[0]
    assert pattern.tolist() == [0, 1, -1, 2, -1] and info["dash"]["dashed"] == 3 and info["dash"]["ignored"] == 0
    assert info["occlude"]["segments"] == len(out[1]) - len(out[2])               # the occlusion works on the dashes
    assert info["occlude"]["hidden"] + info["occlude"]["cut"] > 0                 # and the shape on top cuts them


def test_svg_flow_reads_the_drawing_and_leaves_the_gcode_file_alone():
    from orip import svg as SV
    plain, pinfo = SV.build_stream_from_svg(DC.TOOL_SVG, svg_options([]), want_paths=True, **PD.pens_doubles())
    Z = Recorder(DD.dash_numpy)
    data, info = SV.build_stream_from_svg(DC.TOOL_SVG, svg_options(["--dashes"]), want_paths=True, **dict(PD.pens_doubles(), dash_fn=Z))
    (off, pts, pattern, phase, po, pv), out = Z.calls[0]
    sx = info["scale"][0]
    k = sx * 40.0 * 256
    assert pattern.tolist() == [0, 1, -1, 2, -1]                                  # the circle says none; the rectangle stands outside the group
    assert pv.tolist() == [int(round(v * k)) for v in (4, 2, 1.5, 3, 5, 1.5, 3, 5)] + [int(round(v * 2 * k)) for v in (4, 2)]
    assert phase.tolist() == [0, int(round(2 * k)), 0, int(round(-1 * 2 * k)) % int(pv[8:].sum()), 0]
    assert info["dash"] == dict(out[3], ignored=0) and info["paths"] == out[3]["paths_out"] > pinfo["paths"] and len(data) != len(plain)
    assert np.array_equal(info["fitted_paths"][1], pinfo["fitted_paths"][1])      # the G-code file does not know of the pass
    with_hatch = DC.TOOL_SVG.replace(b'r="15" stroke-dasharray="none"', b'r="15" fill="black"')       # the circle inherits 4 2; its hatch lines stay solid
    Z = Recorder(DD.dash_numpy)
    data, info = SV.build_stream_from_svg(with_hatch, svg_options(["--dashes", "--hatch-spacing-mm", "2"]), **dict(PD.pens_doubles(), dash_fn=Z))
    pattern = Z.calls[0][0][2]
    assert info["hatch"]["segments"] > 3 and pattern[:5].tolist() == [0, 1, 0, 2, -1] and (pattern[5:] == -1).all() and len(pattern) == 5 + info["hatch"]["segments"]


def test_everything_dashed_away_is_the_empty_stream():
    from orip import gcode as GC
    text = "G21 G90\nG0 X10 Y10\nM3\nG1 X12 Y10\nM5\n"                            # 80 steps, wholly inside the gap
    data, info = GC.build_stream_from_gcode(text, gcode_options(["--dash-mm", "5,20", "--dash-offset-mm", "10"]), dash_fn=DD.dash_numpy, **gcode_steps())
    assert data == GC.EMPTY_STREAM and info["dash"]["paths_out"] == 0 and info["paths"] == 0


def test_a_return_that_does_not_hold_is_refused():
    from orip import gcode as GC
    o = gcode_options(["--dash-mm", "3,1.5"])

    def broken(change):
        def fn(*a):
            off, pts, origin, st = DD.dash_numpy(*a)
            return change(np.array(off), np.array(pts), np.array(origin), dict(st))
        return fn

    def repeat(off, pts, origin, st): pts[1] = pts[0]; return off, pts, origin, st
    def backwards(off, pts, origin, st): return off, pts, origin[::-1], st
    def miscount(off, pts, origin, st): st["dashes"] += 1; return off, pts, origin, st
    def more_ink(off, pts, origin, st): st["length_on"] = st["length_in"] + 1; return off, pts, origin, st
    def one_point(off, pts, origin, st): off[1] = 1; return off, pts, origin, st
    for change in (repeat, backwards, miscount, more_ink, one_point):
        with pytest.raises(RuntimeError):
            GC.build_stream_from_gcode(DC.TOOL_GCODE, o, dash_fn=broken(change), **gcode_steps())


def test_the_tools_print_the_dash_line(tmp_path, capsys):
    from orip import gcode as GC, svg as SV
    (tmp_path / "in.gcode").write_text(DC.TOOL_GCODE)
    GC.main([str(tmp_path / "in.gcode"), "-o", str(tmp_path / "out.bin")] + DC.TOOL_GCODE_ARGS, dash_fn=DD.dash_numpy, **gcode_steps())
    assert "[gcode] dash: 3 strokes dashed, " in capsys.readouterr().out
    (tmp_path / "in.svg").write_bytes(DC.TOOL_SVG)
    SV.main_stream([str(tmp_path / "in.svg"), "--no-preview"] + DC.TOOL_SVG_ARGS, dash_fn=DD.dash_numpy, **PD.pens_doubles())
    out = capsys.readouterr().out
    assert "[svg] dash: 3 strokes dashed, " in out and (tmp_path / "in.gcode").read_text().count("M3") == 5
