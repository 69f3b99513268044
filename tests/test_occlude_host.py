"""--occlude on the CPU: the sequential double of tests/occlude_double.py against the hand-worked answers of the rule and against the rule's stated
consequences on the named and on seeded random drawings; the parser's element ordinals; and the whole front door of orip.svg run through the doubles,
with the pass off (nothing changes, the step is never called) and on, alone and together with the hatch, the pens, the clip, the dedup and the merge."""
from fractions import Fraction

import numpy as np
import pytest

import occlude_cases as OC
import occlude_double as OD

CASES = OC.cases()
SMALL = [k for k in sorted(CASES) if k not in ("scatter", "polygon_of_200_edges")]


def run(case):
    return OD.occlude_numpy(*OC.arrays(case))


def lists(off, pts):
    return [[tuple(q) for q in pts[a:b].tolist()] for a, b in zip(off[:-1], off[1:])]


# ------------------------------------------------------------------ the double against the rule
def test_hand_worked_answers():
    for case, out, origin, counts in OC.HAND:
        off, pts, org, st = run(case)
        assert lists(off, pts) == out, case
        if origin is not None:
            assert org.tolist() == origin
        for k, v in counts.items():
            assert st[k] == v, (case, k)
    case, out = OC.HAND_TRIANGLE
    s, o = OC.shifted(case, OC.TRI_SHIFT), [[(x + OC.TRI_SHIFT, y) for x, y in p] for p in out]
    off, pts, _, _ = run(s)
    assert lists(off, pts) == o
    off, pts, _, _ = run(OC.reverse_stroke(s, 0))
    assert lists(off, pts) == [p[::-1] for p in o[::-1]]                      # the same two segments, reversed and in reverse order


def test_argument_errors_of_the_double():
    good = list(OC.arrays(OC.HAND[0][0]))
    OD.occlude_numpy(*good)
    bad = {0: np.array([0, 1]), 1: np.array([[0, 5], [0, 5]]), 2: np.array([-1]), 3: np.array([0, 0]), 4: np.array([[5, 0], [15, 0], [15, 10], [5, OC.TOP + 1]]),
           5: np.array([1 << 30])}
    for k, v in bad.items():
        args = list(good); args[k] = v
        if k == 3:
            args[4] = np.zeros((0, 2), np.int32)
        with pytest.raises(ValueError):
            OD.occlude_numpy(*args)
    two = OC.arrays(([[(0, 5), (20, 5)]], [0], [OC.sq(5, 0, 15, 10), OC.sq(1, 1, 2, 2)], [2, 1]))
    with pytest.raises(ValueError):
        OD.occlude_numpy(*two)                                               # ring_level decreases


def check_consequences(case):
    """consequences 2 and 3 of the rule on one drawing; returns the result"""
    off, pts, org, st = run(case)
    strokes = case[0]
    assert np.all(np.diff(org) >= 0) and (len(org) == 0 or (org.min() >= 0 and org.max() < len(strokes)))
    for k, s in zip(org.tolist(), lists(off, pts)):
        assert len(s) >= 2 and all(a != b for a, b in zip(s[:-1], s[1:]))
        assert all(q in strokes[k] for q in s[1:-1])                          # interior vertices are input vertices
    assert st["whole"] + st["cut"] + st["hidden"] == st["segments"] == sum(len(s) - 1 for s in strokes)
    assert st["pieces"] - st["collapsed"] == st["points_out"] - st["paths_out"]
    assert st["paths_out"] == len(off) - 1 and st["points_out"] == len(pts)
    return off, pts, org, st


def drawn(off, pts):
    return sorted(tuple(sorted((a, b))) for s in lists(off, pts) for a, b in zip(s[:-1], s[1:]))


@pytest.mark.parametrize("name", SMALL)
def test_named_cases(name):
    case = CASES[name]
    off, pts, org, st = check_consequences(case)
    for k in range(len(case[0])):                                             # 5: a reversed stroke draws the same segments
        o2, p2, _, s2 = run(OC.reverse_stroke(case, k))
        assert drawn(o2, p2) == drawn(off, pts) and all(s2[key] == st[key] for key in ("segments", "whole", "cut", "hidden", "pieces", "collapsed"))


def test_expected_shapes_of_the_named_cases():
    st = run(CASES["comb_of_70_teeth"])[3]
    assert st["pieces"] == 71 and st["cut"] == 1
    off, pts, org, st = run(CASES["nothing_above"])
    a = OC.arrays(CASES["nothing_above"])
    assert np.array_equal(off, a[0]) and np.array_equal(pts, a[1]) and org.tolist() == [0, 1] and st["whole"] == st["segments"]      # 1
    off, pts, org, st = run(CASES["no_rings"])
    assert np.array_equal(pts, OC.arrays(CASES["no_rings"])[1]) and org.tolist() == [0, 1]
    assert run(CASES["all_hidden"])[3]["hidden"] == 3 and len(run(CASES["all_hidden"])[1]) == 0
    assert lists(*run(CASES["along_an_edge_partly"])[:2]) == [[(0, 0), (20, 0)], [(20, 10), (15, 10)], [(5, 10), (0, 10)], [(0, 10), (5, 10)], [(15, 10), (30, 10)]]
    assert run(CASES["along_an_edge_wholly"])[3]["whole"] == 3 and run(CASES["along_an_edge_wholly"])[3]["hidden"] == 1
    assert lists(*run(CASES["two_shapes_touch_on_the_stroke"])[:2]) == [[(0, 10), (5, 10)], [(25, 10), (30, 10)], [(30, 10), (25, 10)], [(5, 10), (0, 10)]]
    assert lists(*run(CASES["through_a_reflex_vertex"])[:2])[:2] == [[(0, 10), (5, 10)], [(25, 10), (30, 10)]]
    assert run(CASES["touching_an_apex"])[3]["whole"] == 2
    st = run(CASES["collapsing_piece"])[3]
    assert st["collapsed"] == 2 and st["cut"] == 2 and st["pieces"] == 2 and st["paths_out"] == 0
    assert run(CASES["levels_decide"])[3]["whole"] == 1
    # a cut that falls on a vertex of the stroke ends the output stroke there: the hidden segments between are gone, nothing is joined across them
    assert lists(*run(CASES["cut_at_a_vertex_of_the_stroke"])[:2])[:2] == [[(0, 5), (5, 5)], [(15, 5), (20, 5)]]


def test_the_sliver_has_two_parameters_that_are_one_double():
    strokes, levels, rings, ring_levels = CASES["sliver_at_2_to_30"]
    shapes = OD._shapes(OC.offsets(rings).tolist(), rings[0], ring_levels)
    (a, b), (c, d) = OD.segment_pieces(strokes[0][0], strokes[0][1], shapes)
    assert a == 0 and d == 1 and b < c and float(b) == float(c)               # a 64-bit or floating shortcut sees no hidden stretch
    assert b.denominator == 1 << 30 and c.denominator > 1 << 53
    assert lists(*run(CASES["sliver_at_2_to_30"])[:2]) == [[(0, 0), ((1 << 29) + 1, 1)], [((1 << 29) + 1, 1), (OC.TOP, 1)]]


def hidden_midpoint(case, k, a, b):
    strokes, levels, rings, ring_levels = case
    shapes = OD._shapes(OC.offsets(rings).tolist(), [q for r in rings for q in r], list(ring_levels))
    x, y = Fraction(a[0] + b[0], 2), Fraction(a[1] + b[1], 2)
    return any(OD._inside(edges, x, y) for lv, edges, _ in shapes if lv > levels[k])


def lattice_steps(s):
    out = []
    for (ax, ay), (bx, by) in zip(s[:-1], s[1:]):
        n = max(abs(bx - ax), abs(by - ay)); ux, uy = (bx - ax) // n, (by - ay) // n
        out += [((ax + i * ux, ay + i * uy), (ax + (i + 1) * ux, ay + (i + 1) * uy)) for i in range(n)]
    return out


def test_random_rectilinear_drawings_are_the_exact_complement():
    for seed in range(150):
        case = OC.random_rectilinear(seed)
        off, pts, org, st = check_consequences(case)
        assert st["collapsed"] == 0
        out = lists(off, pts)
        for k, s in enumerate(case[0]):                                       # 4: the visible lattice steps, each once, in order
            want = [(a, b) for a, b in lattice_steps(s) if not hidden_midpoint(case, k, a, b)]
            got = [st_ for o, t in zip(org.tolist(), out) if o == k for st_ in lattice_steps(t)]
            assert got == want, seed
        again = OD.occlude_numpy(off, pts, np.asarray(case[1], np.int32)[org], *OC.arrays(case)[3:])
        assert np.array_equal(again[0], off) and np.array_equal(again[1], pts) and again[2].tolist() == list(range(len(off) - 1))


def test_random_oblique_drawings():
    for seed in range(120):
        case = OC.random_oblique(seed)
        off, pts, org, st = check_consequences(case)
        if seed % 4 == 0:
            for k in range(len(case[0])):
                o2, p2, _, s2 = run(OC.reverse_stroke(case, k))
                assert drawn(o2, p2) == drawn(off, pts) and all(s2[key] == st[key] for key in ("segments", "whole", "cut", "hidden", "pieces", "collapsed")), seed


# ------------------------------------------------------------------ the parser and the whole front door, through the doubles
import merge_cases as MC
import merge_double as MD
import dedup_double as DD
import pens_double as PD
import gcode_double as GD


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def doubles(occ=None):
    import clip_double as CD
    return dict(CD.svg_doubles(), dedup_fn=DD.dedup_numpy, occlude_fn=occ)


def test_the_parser_records_the_element_of_every_subpath():
    from orip import svg as SV
    t = SV.parse_svg(OC.TOOL_SVG)
    assert t.element.tolist() == OC.TOOL_ELEMENTS and t.fill_group.tolist() == OC.TOOL_FILL_GROUPS
    assert SV.parse_svg(OC.TOOL_SVG, "all").fill_group.tolist() == [0, -1, 2, 2, 3, 4]
    sub, lv = SV.occlusion_rings(t)
    assert sub.tolist() == [0, 2, 3] and lv.tolist() == [0, 2, 2]
    old = SV.SegmentTable(t.kind, t.ctrl, t.mat, t.sub_off, t.closed, t.mats, t.canvas_height, t.fill_group, t.stroke_rgb, t.fill_rgb)      # the field comes last, default None
    assert old.element is None
    with pytest.raises(ValueError):
        SV.occlusion_rings(old)
    assert "--occlude" not in SV.build_gcode_argparser().format_help() and "--occlude" in SV.build_stream_argparser().format_help()
    from orip import gcode as GC
    import recording_device as RD
    gcode_steps, svg_steps = RD.doors_take_the_pass_table()
    assert "--occlude" not in GC.STROKE_ARGS and "occlude_fn" not in gcode_steps and "occlude_fn" in svg_steps


def test_without_the_option_nothing_changes_and_the_step_is_never_called():
    from orip import svg as SV
    occ = OC.OccludeDouble()
    args = OC.TOOL_ARGS[1:] + ["--hatch-spacing-mm", "5", "--pen-colors", "#f00,#00f", "--dedup", "--merge-paths"]
    a, ia = SV.build_stream_from_svg(OC.TOOL_SVG, svg_options(args), **doubles(occ))
    b, ib = SV.build_stream_from_svg(OC.TOOL_SVG, svg_options(args), **doubles(None))
    assert a == b and occ.calls == 0 and "occlude" not in ia and ia["dedup"] == ib["dedup"] and ia["merge"] == ib["merge"] and ia["paths"] == ib["paths"]


@pytest.mark.parametrize("extra", [[], ["--hatch-spacing-mm", "5"], ["--pen-colors", "#f00,#00f"], ["--clip"], ["--dedup"], ["--merge-paths"],
                                   ["--hatch-spacing-mm", "5", "--pen-colors", "#f00,#00f", "--dedup", "--merge-paths", "--clip", "--allow-reverse"]])
def test_the_stream_draws_what_the_double_left(extra):
    from orip import svg as SV
    occ = OC.OccludeDouble()
    data, info = SV.build_stream_from_svg(OC.TOOL_SVG, svg_options(OC.TOOL_ARGS + extra), **doubles(occ))
    plain, pinfo = SV.build_stream_from_svg(OC.TOOL_SVG, svg_options(OC.TOOL_ARGS[1:] + extra), **doubles(None))
    assert occ.calls == 1 and info["occlude"] == occ.out[3] and occ.rings[2] == ("--clip" not in extra)
    st = info["occlude"]
    assert st["cut"] > 0 and st["whole"] > 0 and st["draw_steps_out"] < st["draw_steps_in"] and (st["cut"] > 8 or "--hatch-spacing-mm" not in extra)
    left = OC.unit_steps(lists(occ.out[0], occ.out[1]))
    drawn_steps = OC.unit_steps([s for _, s in MC.strokes_of(data)])
    if "--dedup" in extra:
        assert set(drawn_steps) == set(left) and len(drawn_steps) <= len(left)  # what is doubled among what is left goes, pen by pen
        assert "--pen-colors" in extra or len(drawn_steps) == len(set(left))
    else:
        assert sorted(drawn_steps) == sorted(left)
    before = OC.unit_steps([s for _, s in MC.strokes_of(plain)])
    assert set(drawn_steps) < set(before)                                     # ink is only ever taken away
    if "--pen-colors" in extra:                                               # a piece keeps the pen of its stroke: the red path's outline and hatch stay red
        by_pen = lambda d: {c: set(OC.unit_steps([s for k, s in MC.strokes_of(d) if k == c])) for c in (0, 1)}
        now, was = by_pen(data), by_pen(plain)
        assert now[0] <= was[0] and now[1] <= was[1] and now[0] and now[1]
    if "--hatch-spacing-mm" in extra:
        assert info["hatch"]["segments"] > 10
    # the line, element 1, is gone between the outer ring's sides, x in (60, 160): the hole only begins at y = 70, and the rectangle below it hides nothing of it
    sx, _, ox, _ = info["scale"]
    tx = lambda x: int(round((x * sx + ox) * 4))
    line = [s for k, s in zip(occ.out[2].tolist(), lists(occ.out[0], occ.out[1])) if occ.level[k] == 1]
    assert sorted(p[0] for s in line for p in s) == [tx(10), tx(60), tx(160), tx(190)] and all(len(s) == 2 for s in line)


def test_rings_are_converted_as_the_strokes_are():
    m = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=40.0, W=8400, H=11880, invert_y=1)
    off = np.array([0, 4, 7]); mm = np.array([[10.013, 20.0125], [100.4, 20.3], [100.2, 290.0], [10.0, 299.0], [-5.0, 10.0], [50.0125, 10.0], [20.0, 80.0]])
    r_off, r_pts = OD.rings_to_steps(off, mm, [0, 1], m, True)
    w_off, w_pts = GD.to_steps_numpy(off, mm, m)                              # no point of these rings repeats, so the conversion drops none
    assert np.array_equal(r_off, w_off) and np.array_equal(r_pts, w_pts)
    u_off, u_pts = OD.rings_to_steps(off, mm, [0, 1], m, False)
    assert u_pts.min() < 0 and np.array_equal(np.clip(u_pts, 0, [8399, 11879]), r_pts) and not np.array_equal(u_pts, r_pts)


def test_under_clip_a_shape_half_off_the_sheet_still_hides():
    """the reason for the unclamped rings: under --clip the strokes are cut at the sheet's edge, not moved, and so must the shapes be left where they are"""
    from orip import svg as SV
    occ = OC.OccludeDouble()
    data, info = SV.build_stream_from_svg(OC.TOOL_SVG_OFF_SHEET, svg_options(OC.TOOL_ARGS + ["--clip"]), **doubles(occ))
    r_off, r_pts, clamp = occ.rings
    W = info["target"][0]
    assert not clamp and r_pts[:, 0].max() == 330 * 4 > W - 1 and info["clip"]["cut"] >= 1
    out = lists(occ.out[0], occ.out[1])
    first = [s for k, s in zip(occ.out[2].tolist(), out) if k == 0]
    assert first == [[(0, s[0][1]), (150 * 4, s[0][1])] for s in first] and len(first) == 1          # the stroke at y = 80 ends at the triangle's left side and does not come back
    occ2 = OC.OccludeDouble()
    SV.build_stream_from_svg(OC.TOOL_SVG_OFF_SHEET, svg_options(OC.TOOL_ARGS), **doubles(occ2))      # without --clip both are clamped, as the outlines that are drawn
    assert occ2.rings[2] and occ2.rings[1][:, 0].max() == W - 1
