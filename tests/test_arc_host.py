"""--arcs on the host: the rule of orip_gcode_flatten through its sequential double (tests/arc_double.py), the parser with motion modes
(orip.gcode.parse_gcode_arcs), the option checks, and the route through orip.gcode.build_stream_from_gcode with every device step a double.

The bound of the geometric tests, E = 2^-40 r, is a bound on rounding, not a measurement.  With u = 2^-53:
  * a direction is s / n per component with n = sqrt(sx * sx + sy * sy): the two squares and their sum carry (1 + u) each, the square root halves that and
    adds its own u, the division another: every component is off by at most 3.5 u relative, so the length of a direction is within 4 u of 1.  Every level
    of the bisection normalises anew, so this does not grow with the depth; what the levels do accumulate moves a point ALONG the circle only.
  * rho is rA exactly when rA == rB ((rB - rA) * t is 0).  rho * u carries one more u per component: the offset from the centre is within 5 u r of r.
  * C + rho * u rounds once per coordinate, by at most u |P|, and |P| <= |C| + r <= (2^8 + 1) r in every case of tests/arc_cases.py: 1.5 * 2^8 u r.
  * the reference radius rA itself is off from |A - C| by 2.5 u r, and a = A - C by one rounding per component of a value below (2^8 + 1) r.
Together below 2^10 u r = 2^-43 r; 2^-40 r leaves a factor of eight, and is far below any tolerance a depth m <= 16 admits (about 2^-34 r).
The distances themselves are taken in exact rational arithmetic, so the check adds no rounding of its own."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import arc_cases as AC
import arc_double as AD

SMALL = AC.small_cases()
ALL = dict(SMALL, **{f"random_{s}": AC.random_case(s) for s in AC.RANDOM_SEEDS})
E = F(1, 1 << 40)


def arcs_of(case, equal_radii=False):
    """(Arc, its points with A in front) of every arc of a case; equal_radii: only those whose radii agree to 2^-48 r (the inputs made with sin / cos do)"""
    kind, seg, _off, tol = case
    for kd, s in zip(kind.tolist(), seg.tolist()):
        if kd == AC.LINE:
            continue
        a = AD.Arc(kd, (s[0], s[1]), (s[2], s[3]), (s[4], s[5]), tol)
        if equal_radii and abs(a.rA - a.rB) > max(a.rA, a.rB) * 2.0 ** -48:
            continue
        yield a, [a.A] + a.points()


def dist2(P, C):
    return (F(P[0]) - F(C[0])) ** 2 + (F(P[1]) - F(C[1])) ** 2


@pytest.mark.parametrize("name", sorted(ALL))
def test_points_lie_on_the_circle(name):
    seen = 0
    for a, pts in arcs_of(ALL[name], True):
        r = F(max(a.rA, a.rB)); lo, hi = (r * (1 - E)) ** 2, (r * (1 + E)) ** 2
        for P in pts:
            assert lo <= dist2(P, a.C) <= hi, (name, P)
        seen += 1
    assert seen or name in ("lines_only", "radii_differ", "same_ray")


@pytest.mark.parametrize("name", sorted(ALL))
def test_chords_stay_within_the_tolerance_and_one_level_less_would_not(name):
    tol = F(ALL[name][3])
    for a, pts in arcs_of(ALL[name], True):
        r = F(max(a.rA, a.rB)); inner = (r - tol - E * r) ** 2
        for P, Q in zip(pts[:-1], pts[1:]):
            M = ((F(P[0]) + F(Q[0])) / 2, (F(P[1]) + F(Q[1])) / 2)
            assert (M[0] - F(a.C[0])) ** 2 + (M[1] - F(a.C[1])) ** 2 >= inner, (name, P, Q)
        if a.m > 0:
            b = AD.Arc(a.kind, a.A, a.B, a.C, float(tol), force_m=a.m - 1)
            coarse = [b.A] + b.points()
            worst = min((((F(P[0]) + F(Q[0])) / 2 - F(a.C[0])) ** 2 + ((F(P[1]) + F(Q[1])) / 2 - F(a.C[1])) ** 2) for P, Q in zip(coarse[:-1], coarse[1:]))
            assert worst < inner, (name, a.m)


@pytest.mark.parametrize("name", sorted(ALL))
def test_first_and_last_points_are_the_files(name):
    kind, seg, sub_off, tol = ALL[name]
    off, pts, st = AD.flatten((kind, seg, sub_off), tol)
    assert len(off) == len(sub_off) and off[0] == 0 and off[-1] == len(pts)
    for p in range(len(sub_off) - 1):
        assert pts[off[p]].view(np.int64).tolist() == seg[sub_off[p], 0:2].view(np.int64).tolist()
        assert pts[off[p + 1] - 1].view(np.int64).tolist() == seg[sub_off[p + 1] - 1, 2:4].view(np.int64).tolist()
    for a, apts in arcs_of(ALL[name]):
        assert apts[0] == a.A and apts[-1] == a.B and len(apts) == a.N + 1
    assert st["arcs"] == int((kind >= 2).sum()) and st["pieces"] == len(pts) - (len(sub_off) - 1) - int((kind == 1).sum())


@pytest.mark.parametrize("name", sorted(ALL))
def test_a_mirrored_clockwise_arc_is_the_mirrored_counter_clockwise_arc(name):
    kind, seg, sub_off, tol = ALL[name]
    mseg = seg * np.array([1.0, -1.0] * 3)
    mkind = np.where(kind == 1, 1, 5 - kind).astype(np.int32)
    off, pts, _ = AD.flatten((kind, seg, sub_off), tol)
    moff, mpts, _ = AD.flatten((mkind, mseg, sub_off), tol)
    assert np.array_equal(off, moff)
    want = pts * np.array([1.0, -1.0])
    assert np.array_equal(np.where(want == 0.0, 0.0, want).view(np.int64), np.where(mpts == 0.0, 0.0, mpts).view(np.int64))      # but for the sign of a zero, bit for bit


def test_a_full_circle_returns_to_its_start_in_four_spans():
    for name in ("full_cw", "full_ccw_oblique"):
        (a, pts), = arcs_of(SMALL[name])
        assert a.full and a.S == 4 and a.N == 4 << a.m and len(pts) == a.N + 1 and pts[0] == pts[-1] == a.A
        assert a.J[4] == a.J[0]
    (a, pts), = arcs_of(SMALL["full_cw"])
    assert a.m == 4 and pts[16] == (5.0, -5.0) and pts[32] == (0.0, 0.0) and pts[48] == (5.0, 5.0)      # clockwise from (10, 0) about (5, 0): the joint q1 lies below the centre


def test_the_depths_and_spans_of_the_named_cases():
    want = {"quarter_ccw": (1, 4), "quarter_cw": (1, 4), "three_quarters_ccw": (3, 4), "half_ccw": (2, 4), "hair_over_90_ccw": (2, 4), "hair_under_90_cw": (1, 4),
            "hair_over_180_cw": (3, 4), "hair_over_270_ccw": (4, 4), "hair_under_360_ccw": (4, 4), "hair_over_0_cw": (1, 0), "short_m0": (1, 0), "short_m1": (1, 1),
            "block_inside_a_span": (2, 11), "r_form_short": (2, 4), "r_form_long": (3, 4), "same_ray": (0, 0)}
    for name, (S, m) in want.items():
        a, _ = next(arcs_of(SMALL[name]))
        assert (a.S, a.m) == (S, m), name
    assert len(AD.flatten(SMALL["block_of_segments"][:3], 0.02)[0]) == 301


def test_what_the_rule_rejects():
    k, s, o, tol = SMALL["quarter_ccw"]
    for bad_tol in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(AD.FlattenError) as e:
            AD.flatten((k, s, o), bad_tol)
        assert e.value.what == "tol"
    for kd in (0, 4):
        with pytest.raises(AD.FlattenError) as e:
            AD.flatten((np.array([kd]), s, o), tol)
        assert e.value.what == "kind"
    for what, seg in (("finite", [15.0, 10.0, 10.0, 15.0, float("nan"), 10.0]), ("finite", [float("inf"), 10.0, 10.0, 15.0, 10.0, 10.0]), ("radius", [15.0, 10.0, 10.0, 15.0, 15.0, 10.0]),
                      ("radius", [15.0, 10.0, 10.0, 15.0, 10.0, 15.0]), ("finite", [1e200, 0.0, 0.0, 1e200, 0.0, 0.0])):
        with pytest.raises(AD.FlattenError) as e:
            AD.flatten((k, np.array([seg]), o), tol)
        assert e.value.what == what, seg
    with pytest.raises(AD.FlattenError) as e:
        AD.flatten((k, np.array([[1e9, 0.0, 0.0, 1e9, 0.0, 0.0]]), o), 1e-9)         # r (1 - c_16) = 1e9 * 7e-11 > tol
    assert e.value.what == "depth"
    with pytest.raises(AD.FlattenError) as e:
        AD.flatten((np.array([1, 1]), np.array([[0.0, 0, 1, 1, 0, 0], [1.0, 1.5, 2, 2, 0, 0]]), np.array([0, 2])), tol)
    assert e.value.what == "chain"


# ------------------------------------------------------------------ the parser
def parse(text, pens=None):
    from orip import gcode as GC
    return GC.parse_gcode_arcs(text, pens)


def rows(t):
    return [(int(k), *[round(v, 9) for v in s]) for k, s in zip(t.kind, t.seg.tolist())]


def test_modal_g2_then_bare_lines():
    t, moves = parse("G0 X10 Y0\nM3\nG2 X0 Y-10 I-10 J0\nX-10 Y0 I0 J10\nG1 X-10 Y5\nG3 X-5 Y5 I2.5\nM5\n")
    assert rows(t) == [(2, 10, 0, 0, -10, 0, 0), (2, 0, -10, -10, 0, 0, 0), (1, -10, 0, -10, 5, 0, 0), (3, -10, 5, -5, 5, -7.5, 5)]
    assert t.sub_off.tolist() == [0, 4] and moves == 4
    t, _ = parse("M3\nG1 X1 G3 X2 Y0 I1\n")                               # the last motion word of a line wins
    assert rows(t) == [(3, 0, 0, 2, 0, 1, 0)]
    t, _ = parse("M3\nG3 X2 Y0 I1 G1\nX5\n")
    assert rows(t) == [(1, 0, 0, 2, 0, 0, 0), (1, 2, 0, 5, 0, 0, 0)]


def test_g91_1_leaves_the_distance_mode_alone_and_g90_1_makes_centres_absolute():
    from orip import gcode as GC
    text = "G90 G91.1\nG0 X10 Y10\nM3\nG1 X20 Y10\nG3 X20 Y20 I0 J5\nM5\n"
    t, _ = parse(text)
    assert rows(t) == [(1, 10, 10, 20, 10, 0, 0), (3, 20, 10, 20, 20, 20, 15)]
    off, pts, _ = GC.parse_gcode(text)                                      # the old parser reads G91.1 as G91: relative from there on
    assert pts.tolist() == [[10, 10], [30, 20], [50, 40]]
    t, _ = parse("G90.1\nG0 X20 Y10\nM3\nG3 X20 Y20 I20 J15\nG2 X25 Y15 J15\nG91.1\nG2 X20 Y10 I-5\nM5\n")
    assert rows(t) == [(3, 20, 10, 20, 20, 20, 15), (2, 20, 20, 25, 15, 20, 15), (2, 25, 15, 20, 10, 20, 15)]      # under G90.1 a missing I is A's x: here 20
    t, _ = parse("G91\nG0 X10 Y10\nM3\nG3 X0 Y10 I0 J5\nM5\n")              # G91: the end point is relative, the centre an offset as ever
    assert rows(t) == [(3, 10, 10, 10, 20, 10, 15)]


def test_inches():
    t, _ = parse("G20\nG0 X1 Y0\nM3\nG3 X0 Y1 I-1 J0\nG21\nG1 X0 Y0\nG20 G2 X1 Y1 R1\nM5\n")
    assert rows(t)[0] == (3, 25.4, 0, 0, 25.4, 0, 0) and rows(t)[1] == (1, 0, 25.4, 0, 0, 0, 0)
    k, ax, ay, bx, by, cx, cy = rows(t)[2]
    assert (k, ax, ay, bx, by) == (2, 0, 0, 25.4, 25.4) and (round(cx, 6), round(cy, 6)) in ((0.0, 25.4), (25.4, 0.0))


def test_an_i_only_full_circle_and_the_issues_example():
    t, moves = parse("G0 X10 Y0\nM3\nG2 I-5\nM5\n")
    assert rows(t) == [(2, 10, 0, 10, 0, 5, 0)] and moves == 1
    t, moves = parse("G0 X10 Y0\nM3\nG2 X10 Y0 I-5 J0\nM5\n")
    assert rows(t) == [(2, 10, 0, 10, 0, 5, 0)]
    off, pts, st = AD.flatten(t, 0.0125)
    assert st == {"arcs": 1, "pieces": 64, "full_circles": 1} and pts[32].tolist() == [0.0, 0.0]
    t, _ = parse("G0 X10 Y0\nM3\nG1 I-5\nM5\n")                             # in mode G1 a line without X or Y does not move
    assert len(t.kind) == 0 and t.sub_off.tolist() == [0]


def test_the_r_form():
    t, _ = parse("G0 X0 Y0\nM3\nG3 X10 Y0 R6\nM5\nM3\nG2 X0 Y0 R6\nM5\nM3\nG3 X10 Y0 R-6\nM5\nM3\nG2 X0 Y0 R-6\nM5\n")
    h = math.sqrt(36 - 25)
    c = [(round(r[5], 9), round(r[6], 9)) for r in rows(t)]
    assert c == [(5, round(h, 9)), (5, round(h, 9)), (5, round(-h, 9)), (5, round(-h, 9))]      # G3 R > 0: left of A -> B; G2 back: right of B -> A, the same side; R < 0: the others
    for name, sweeps in (("r_form_short", 2), ("r_form_long", 3)):
        assert [a.S for a, _ in arcs_of(SMALL[name])] == [sweeps, sweeps]
    t, _ = parse("G0 X0 Y0\nM3\nG2 X10 Y0 R4.996\nM5\n")                     # short by 0.004 mm: the centre is the midpoint
    assert rows(t) == [(2, 0, 0, 10, 0, 5, 0)]


@pytest.mark.parametrize("text, line, what", [
    ("G0 X0 Y0\nM3\n\nG2 X10 Y0 R4.99\n", 4, "too short"),
    ("M3\nG2 X0 Y0 R5\n", 2, "no centre"),
    ("M3\nG2 X10 Y0 R0\n", 2, "R0"),
    ("M3\nG2 X10 Y0 R6 I5\n", 2, "both R and I"),
    ("; header\nM3\nG2 X10 Y0\n", 3, "on its centre"),
    ("M3\nG3 X10 Y0 I10 J0\n", 2, "on its centre"),
    ("G0 X10 Y0\nM3\nG1 X10 Y0\n(comment)\nG3 X0 Y10.6 I-10 J0\n", 5, "radii"),
    ("G0 X10 Y0\nG3 X0 Y10.02 I-10 J0\n", 2, "radii"),
    ("G18\nM3\nG1 X5\nG2 X10 Y0 I2.5\n", 4, "G18"),
    ("G19 G0 X1\nG3 I1\n", 2, "G19"),
])
def test_every_error_names_its_line(text, line, what):
    with pytest.raises(ValueError, match=f"line {line}: .*{what}"):
        parse(text)


def test_the_radius_limits():
    parse("G0 X10 Y0\nM3\nG3 X0 Y10.004 I-10 J0\n")                         # 0.004 mm: under the small limit
    parse("G0 X1000 Y0\nM3\nG3 X0 Y1000.4 I-1000 J0\n")                     # 0.4 mm, under a thousandth of 1000 mm
    with pytest.raises(ValueError, match="line 3"):
        parse("G0 X1000 Y0\nM3\nG3 X0 Y1000.6 I-1000 J0\n")                 # over 0.5 mm
    with pytest.raises(ValueError, match="line 3"):
        parse("G0 X1 Y0\nM3\nG3 X0 Y1.006 I-1 J0\n")                        # over 0.005 mm and over a thousandth
    parse("G17\nG18\nG1 X1\nG17\nM3\nG2 X2 I0.5\n")                         # G18 alone is no error, and G17 restores the plane


def test_an_arc_with_the_pen_up_only_moves_the_cursor():
    t, moves = parse("G0 X10 Y0\nG3 X0 Y10 I-10\nM3\nG1 X0 Y20\nM5\nG2 X5 Y25 I5\nM3\nG1 X6 Y25\n")
    assert rows(t) == [(1, 0, 10, 0, 20, 0, 0), (1, 5, 25, 6, 25, 0, 0)] and t.sub_off.tolist() == [0, 1, 2] and moves == 2


def test_pens_through_pens_out_and_the_z_rule():
    pens = []
    t, _ = parse("T2\nG0 X0 Y0\nZ-1\nG2 X10 Y0 I5\nT5\nG1 X20\nZ1\nG0 X30\nZ0 F300\nG3 X40 Y0 I5 K2 P1\nM5\n", pens)
    assert pens == [2, 5] and t.sub_off.tolist() == [0, 2, 3] and t.kind.tolist() == [2, 1, 3]
    with pytest.raises(ValueError, match="T9"):
        parse("T9\n", [])
    parse("T9\n")                                                           # without pens_out a T word is skipped, as in parse_gcode


# ------------------------------------------------------------------ the old paths, the options, the route
def test_the_old_parser_still_draws_chords():
    from orip import gcode as GC
    off, pts, moves = GC.parse_gcode(AC.TOOL_GCODE)
    assert off.tolist() == [0, 3, 12] and moves == 10
    assert pts[:3].tolist() == [[60, 50], [40, 50], [60, 50]] and pts[3:6].tolist() == [[85, 40], [115, 40], [120, 45]]
    off, pts, moves = GC.parse_gcode("G0 X10 Y0\nM3\nG2 X10 Y0 I-5 J0\nM5\n")
    assert pts.tolist() == [[10, 0], [10, 0]]                               # the full circle is a move of length zero there


def _doubles(**more):
    import clip_double as CD
    return dict(CD.gcode_doubles(), **more)


def test_arcs_on_an_arc_free_text_changes_nothing_and_flattens_nothing():
    from orip import gcode as GC
    import clip_cases as CC

    def never(*_a):
        raise AssertionError("flatten_fn called")
    for text in (CC.circle_gcode(), "G91.1\nG0 X1 Y1\nM3\nG1 X5 Y5\nX9 Y2\nM5\n"):
        for kw in ({}, {"clip": True}, {"tool_pens": True}):
            want, winfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(**kw), **_doubles())
            got, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(arcs=True, **kw), **_doubles(flatten_fn=never))
            assert got == want and "arcs" not in info and info["paths_mm"] == winfo["paths_mm"] and info["pen_down_moves"] == winfo["pen_down_moves"]


def test_the_route_with_arcs_equals_the_flattened_paths_fed_directly():
    from orip import gcode as GC
    import merge_cases as MC
    o = GC.GcodeOptions(arcs=True)
    tol = GC.arc_tolerance(o)
    assert tol == 0.5 / 40.0
    t, moves = GC.parse_gcode_arcs(AC.TOOL_GCODE)
    off, pts, st = AD.flatten(t, tol)
    for kw in ({}, {"clip": True, "clip_margin_mm": 45.0}, {"loop_start": True, "no_reorder": True}):
        more = dict(seam_fn=_seams()) if kw.get("loop_start") else {}
        want, winfo = GC.build_stream_from_gcode((off, pts), GC.GcodeOptions(**kw), **_doubles(**more))
        got, info = GC.build_stream_from_gcode(AC.TOOL_GCODE, GC.GcodeOptions(arcs=True, **kw), **_doubles(flatten_fn=AD.flatten_fn, **more))
        assert got == want and info["arcs"] == dict(st, tolerance_mm=tol) and info["pen_down_moves"] == moves == 10 and info["paths_mm"] == 2
    chords, cinfo = GC.build_stream_from_gcode(AC.TOOL_GCODE, GC.GcodeOptions(), **_doubles())
    arcs, ainfo = GC.build_stream_from_gcode(AC.TOOL_GCODE, GC.GcodeOptions(arcs=True), **_doubles(flatten_fn=AD.flatten_fn))
    assert ainfo["paths"] == cinfo["paths"] == 2
    a, c = MC.strokes_of(arcs), MC.strokes_of(chords)
    assert len(a) == len(c) == 2 and sum(len(p) - 1 for _, p in a) > sum(len(p) - 1 for _, p in c)      # steps count max(|dx|, |dy|): the circle's 4 sqrt(2) r against two diameters drawn on top of each other, the fillets against their chords


def _seams():
    import seam_double as SM
    return SM.seams


def test_argument_errors():
    from orip import gcode as GC
    with pytest.raises(ValueError, match="--arc-tolerance-mm needs --arcs"):
        GC.arc_tolerance(GC.GcodeOptions(arc_tolerance_mm=0.1))
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="positive finite"):
            GC.arc_tolerance(GC.GcodeOptions(arcs=True, arc_tolerance_mm=bad))
    assert GC.arc_tolerance(GC.GcodeOptions()) is None
    assert GC.arc_tolerance(GC.GcodeOptions(arcs=True, arc_tolerance_mm=0.25)) == 0.25
    assert GC.arc_tolerance(GC.GcodeOptions(arcs=True, steps_per_mm=80.0, scale_x=-2.0, scale_y=0.5)) == 0.5 / (80.0 * 2.0)
    with pytest.raises(ValueError, match="--arc-tolerance-mm needs --arcs"):
        GC.build_stream_from_gcode("M3\nG1 X1\n", GC.GcodeOptions(arc_tolerance_mm=0.1), **_doubles())
    with pytest.raises(ValueError, match="--arc-tolerance-mm needs --arcs"):
        GC.main(["in.gcode", "--arc-tolerance-mm", "0.1"])
    with pytest.raises(ValueError, match="positive finite"):
        GC.main(["in.gcode", "--arcs", "--arc-tolerance-mm", "0"])
    a = GC.build_argparser().parse_args(["in.gcode"])
    assert a.arcs is False and a.arc_tolerance_mm is None
    a = GC.options_from_args(GC.build_argparser().parse_args(["in.gcode", "--arcs", "--arc-tolerance-mm", "0.02"]))
    assert a.arcs is True and a.arc_tolerance_mm == 0.02
