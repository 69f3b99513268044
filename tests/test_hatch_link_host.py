"""--hatch-connect on the CPU: the sequential double (tests/hatch_link_double.py) keeps every consequence include/orip.h draws from the rule on the named
drawings of tests/hatch_link_cases.py; the square is worked by hand; and svg2stream's plumbing runs with the double injected as hatch_link_fn: the option
errors, the unchanged stream without the option, pens and levels following a zigzag's first line, the occlusion cutting a zigzag, the unchanged G-code."""
import numpy as np
import pytest

import hatch_link_cases as LC
import hatch_link_double as LD
import merge_cases as MC
import occlude_cases as OC

CASES = LC.cases()


def run(name):
    return LD.hatch_link(*LC.args(CASES[name]))


def lists(off, pts):
    return [[tuple(q) for q in pts[a:b].tolist()] for a, b in zip(off[:-1], off[1:])]


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_double_keeps_the_consequences(name):
    LC.check_consequences(CASES[name], run(name))


def test_the_square_by_hand():
    """rows y = 120, 160, .., 1080: 25 lines from x = 127 to x = 1073, every other one backwards; every link runs 40 steps straight up inside the square"""
    off, pts, moff, member, st = run("square")
    want = []
    for k, y in enumerate(range(120, 1100, 40)):
        want += [(127, y), (1073, y)] if k % 2 == 0 else [(1073, y), (127, y)]
    assert lists(off, pts) == [want] and moff.tolist() == [0, 25] and member.tolist() == list(range(25))
    assert st == dict(lines=25, in_reach=24, eligible=24, links=24, coincident=0, paths_out=1, points_out=50, link_steps=960)


def test_the_counts_the_rule_was_chosen_by():
    """lines in -> strokes out of the shapes the rule was tried on, and the refusals of the slit"""
    for name, lines, strokes in (("square", 25, 1), ("l_shape", 30, 1), ("u_shape", 50, 2), ("circle_64", 49, 5), ("ring_with_hole", 69, 7), ("cross_hatch", 50, 2)):
        st = run(name)[4]
        assert (st["lines"], st["paths_out"]) == (lines, strokes), name
    off, pts, moff, member, st = run("slit")
    assert (st["lines"], st["in_reach"], st["eligible"], st["paths_out"]) == (35, 40, 33, 2) and np.diff(moff).tolist() == [20, 15]
    c = CASES["slit"]                                                        # the 7 refused pairs run along one row across the slit
    refused = 0
    for a in range(35):
        for b in range(a + 1, 35):
            e, s = c["pts"][2 * a + 1], c["pts"][2 * b]
            if ((s - e) ** 2).sum() <= 80 * 80 and e[1] == s[1]:
                refused += 1
                assert e[0] < 600 < s[0] or s[0] < 600 < e[0]
    assert refused == 7


def test_families_shapes_inset_and_reach():
    c, (off, pts, moff, member, st) = CASES["cross_hatch"], run("cross_hatch")
    assert [sorted(set(c["cls"][member[a:b]].tolist())) for a, b in zip(moff[:-1], moff[1:])] == [[0], [1]]       # the families never mix
    c, (off, pts, moff, member, st) = CASES["two_squares"], run("two_squares")
    ends, starts = c["pts"][1::2][c["cls"] == 0], c["pts"][0::2][c["cls"] == 2]
    assert min(int(((s - e) ** 2).sum()) for e in ends for s in starts) <= 80 * 80                               # ends across the gap lie within reach,
    assert st["paths_out"] == 2 and [sorted(set(c["cls"][member[a:b]].tolist())) for a, b in zip(moff[:-1], moff[1:])] == [[0], [2]]      # and nothing links between shapes
    for name in ("inset_0", "reach_39", "no_serpentine", "no_class", "no_rings", "shape_without_rings", "class_of_one_line"):
        c, (off, pts, moff, member, st) = CASES[name], run(name)
        assert st["links"] == 0 and np.array_equal(off, c["off"]) and np.array_equal(pts, c["pts"]) and member.tolist() == list(range(len(off) - 1)), name
    assert run("inset_0")[4]["in_reach"] == 24 and run("reach_39")[4]["in_reach"] == 0 and run("reach_40")[4]["links"] == 24      # d^2 == reach^2 is in reach
    assert run("empty")[4] == dict.fromkeys(LD.STATS, 0) and run("empty")[0].tolist() == [0]


def test_the_small_print():
    assert run("tie_from_one_end")[3].tolist() == [0, 1, 2] and np.diff(run("tie_from_one_end")[2]).tolist() == [2, 1]      # END 0 has STARTs 1 and 2 at 40: the lower one
    off, pts, moff, member, st = run("tie_from_one_start")
    assert member.tolist() == [0, 2, 1] and np.diff(moff).tolist() == [2, 1]                                                # START 2 has ENDs 0 and 1 at 40: the lower one
    off, pts, moff, member, st = run("not_mutual")
    assert member.tolist() == [0, 1, 2] and np.diff(moff).tolist() == [1, 2] and st["eligible"] == 2 and st["links"] == 1   # 0's best is 2, 2's best is 1: 0 stays single
    off, pts, moff, member, st = run("coincident")
    assert lists(off, pts) == [[(100, 500), (500, 500), (500, 700), (500, 730), (100, 730)]] and st["coincident"] == 1 and st["link_steps"] == 30
    off, pts, moff, member, st = run("three_points_take_no_part")
    assert st["lines"] == 2 and member.tolist() == [0, 2, 1] and lists(off, pts)[1] == [(500, 540), (300, 550), (100, 540)]
    off, pts, moff, member, st = run("mixed_with_outlines")
    assert member.tolist() == [0, 1, 3, 4, 2] and np.diff(moff).tolist() == [1, 3, 1]                                       # strokes that take no part stay at their place
    off, pts, moff, member, st = run("many_starts")
    assert st["in_reach"] == st["eligible"] == 70 and st["links"] == 1 and member[:2].tolist() == [0, 1]
    assert [run(k)[4]["links"] for k in ("far_corner_open", "far_corner_outside", "far_corner_on_edge")] == [2, 1, 1]
    assert len(CASES["polygon_of_70_edges"]["ring_pts"]) == 70 and len(CASES["polygon_of_3000_edges"]["ring_pts"]) == 3000
    st = run("random_lines")[4]
    assert st["in_reach"] > 50 and 0 < st["links"] < st["eligible"] < st["in_reach"]                                       # refusals, ties and losers all occur


def test_bad_arguments_of_the_double():
    c = CASES["square"]
    for bad in (dict(reach=0), dict(reach=(1 << 20) + 1), dict(cls=np.full(25, -2)), dict(ring_group=np.array([1, 0]), ring_off=np.array([0, 2, 4]))):
        with pytest.raises(ValueError):
            LD.hatch_link(*LC.args(dict(c, **bad)))


# ------------------------------------------------------------------ the front door, through the doubles
def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def doubles(link=None, occ=None):
    import clip_double as CD
    import dedup_double as DD
    return dict(CD.svg_doubles(), dedup_fn=DD.dedup_numpy, occlude_fn=occ, hatch_link_fn=link)


def pen_lifts(data):
    return len(MC.strokes_of(data))


def test_the_options():
    from orip import svg as SV
    from orip import gcode as GC
    reach = lambda args: SV.hatch_connect_reach(svg_options(args))
    assert reach(LC.TOOL_ARGS) is None and reach(LC.TOOL_ARGS + ["--hatch-connect"]) == 80 and reach(LC.TOOL_ARGS + ["--hatch-connect", "--hatch-connect-mm", "3.04"]) == 30
    for bad in (["--hatch-connect"], ["--hatch-connect", "--hatch-connect-mm", "5"], LC.TOOL_ARGS + ["--hatch-connect-mm", "5"], ["--hatch-connect-mm", "5"],
                LC.TOOL_ARGS + ["--hatch-connect", "--hatch-connect-mm", "0"], LC.TOOL_ARGS + ["--hatch-connect", "--hatch-connect-mm", "-1"],
                LC.TOOL_ARGS + ["--hatch-connect", "--hatch-connect-mm", "nan"], LC.TOOL_ARGS + ["--hatch-connect", "--hatch-connect-mm", "inf"],
                LC.TOOL_ARGS + ["--hatch-connect", "--hatch-connect-mm", "0.04"], LC.TOOL_ARGS + ["--hatch-connect", "--hatch-connect-mm", "200000"]):
        with pytest.raises(ValueError, match="hatch-connect"):
            reach(bad)
        with pytest.raises(ValueError, match="hatch-connect"):
            SV.build_stream_from_svg(LC.TOOL_SVG, svg_options(bad), **doubles(LC.HatchLinkDouble()))
    assert "--hatch-connect" in SV.build_stream_argparser().format_help() and "--hatch-connect" not in SV.build_gcode_argparser().format_help()
    import recording_device as RD
    gcode_steps, svg_steps = RD.doors_take_the_pass_table()
    assert "--hatch-connect" not in GC.build_argparser().format_help() and "hatch_link_fn" not in gcode_steps and "hatch_link_fn" in svg_steps


def test_without_the_option_nothing_changes_and_the_step_is_never_called():
    from orip import svg as SV
    link = LC.HatchLinkDouble()
    args = LC.TOOL_ARGS + ["--pen-colors", "#f00,#00f", "--dedup", "--merge-paths", "--occlude"]
    a, ia = SV.build_stream_from_svg(LC.TOOL_SVG, svg_options(args), **doubles(link, OC.OccludeDouble()))
    b, ib = SV.build_stream_from_svg(LC.TOOL_SVG, svg_options(args), **doubles(None, OC.OccludeDouble()))
    assert a == b and link.calls == 0 and "hatch_link" not in ia and ia["paths"] == ib["paths"] and ia["occlude"] == ib["occlude"]


@pytest.mark.parametrize("extra", [[], ["--clip"], ["--pen-colors", "#f00,#00f"], ["--hatch-direction", "cross"], ["--hatch-angle-deg", "30", "--hatch-direction", "cross"],
                                   ["--invert-y", "1"], ["--merge-paths", "--dedup", "--simplify-mm", "0", "--allow-reverse", "--pen-colors", "#f00,#00f"]])
def test_the_stream_draws_the_zigzags(extra):
    from orip import svg as SV
    link = LC.HatchLinkDouble()
    dbl = doubles(link)
    if "--simplify-mm" in extra:
        dbl["simplify_fn"] = __import__("simplify_double").simplify_numpy
    if "--hatch-angle-deg" in extra:
        hatch = __import__("hatch_angle_double").HatchAngleWithGroups()
        dbl.update(hatch_fn=hatch.hatch, hatch_groups_fn=hatch.hatch_groups)
    data, info = SV.build_stream_from_svg(LC.TOOL_SVG, svg_options(LC.TOOL_ARGS + ["--hatch-connect"] + extra), **dbl)
    plain, pinfo = SV.build_stream_from_svg(LC.TOOL_SVG, svg_options(LC.TOOL_ARGS + extra), **dict(dbl, hatch_link_fn=None))
    st = info["hatch_link"]
    assert link.calls == 1 and st == dict(link.out[4], reach=80) and link.rings[3] == ("--clip" not in extra) and link.rings[2].tolist() == [0, 1, 2]
    assert st["lines"] == info["hatch"]["segments"] == int((link.cls >= 0).sum()) and st["links"] > 0.8 * st["lines"]
    families = 2 if "cross" in extra else 1
    assert sorted(set((link.cls[link.cls >= 0] & 1).tolist())) == list(range(families)) and sorted(set((link.cls[link.cls >= 0] >> 1).tolist())) == [0, 1, 2]
    LC.check_consequences(dict(off=link.inp[0], pts=link.inp[1], cls=link.cls, ring_off=link.rings[0], ring_pts=link.rings[1], ring_group=link.rings[2], reach=80), link.out)
    if "--merge-paths" not in extra:
        assert pen_lifts(data) == pen_lifts(plain) - st["links"] == st["paths_out"]
        if "--hatch-angle-deg" not in extra:                                  # axis-parallel throughout: the drawing is the plain one and the links, step for step
            assert sorted(OC.unit_steps([s for _, s in MC.strokes_of(data)])) == sorted(OC.unit_steps([s for _, s in MC.strokes_of(plain)]) + link_unit_steps(link))
    else:
        assert pen_lifts(data) < pen_lifts(plain) - st["links"] // 2
    assert any(line.startswith("[svg] hatch connect: ") and f"{st['links']} links" in line for line in __import__("orip.gcode").gcode.report_lines("svg", info))


def link_unit_steps(link):
    """the unit steps of the links themselves: what the pass adds to the drawing (axis-parallel or diagonal links only)"""
    off, pts, moff, member, _ = link.out
    i_off, i_pts = link.inp
    out = []
    for a, b in zip(moff[:-1], moff[1:]):
        mem = member[a:b].tolist()
        out += [[tuple(i_pts[i_off[p] + 1].tolist()), tuple(i_pts[i_off[q]].tolist())] for p, q in zip(mem[:-1], mem[1:])]
    return OC.unit_steps([s for s in out if s[0] != s[1]])


def test_pens_and_levels_follow_the_first_line_and_the_occlusion_cuts_a_zigzag():
    from orip import svg as SV
    link, occ = LC.HatchLinkDouble(), OC.OccludeDouble()
    args = LC.TOOL_ARGS + ["--hatch-connect", "--occlude", "--pen-colors", "#f00,#00f"]
    data, info = SV.build_stream_from_svg(LC.TOOL_SVG, svg_options(args), **doubles(link, occ))
    off, pts, moff, member, st = link.out
    assert link.calls == 1 and occ.calls == 1 and len(occ.level) == st["paths_out"]
    first = member[moff[:-1]]
    g = np.where(link.cls >= 0, link.cls >> 1, -1)
    zig = np.diff(moff) > 1
    assert zig.sum() >= 3 and (occ.level[zig] == g[first][zig]).all()                        # a zigzag's level is its shape's, through its first line
    assert info["occlude"]["cut"] > 0
    cut = [k for k in range(len(occ.out[2])) if zig[occ.out[2][k]]]
    o_off = occ.out[0]
    assert len(cut) > int(zig.sum()) and max(o_off[k + 1] - o_off[k] for k in cut) > 2      # the rectangle on top leaves the L's zigzag in several strokes, corners and all
    pens = {c for c, _ in MC.strokes_of(data)}
    assert pens == {0, 1}
    red = [s for c, s in MC.strokes_of(data) if c == 0]                                     # the red rectangle's outline and its one zigzag
    assert len(red) == 2 and all(1300 <= x <= 1800 for s in red for x, _ in s)             # (the fit moves the drawing 10 mm to the left)


def test_the_gcode_file_does_not_know_of_the_pass(tmp_path):
    from orip import svg as SV
    src = tmp_path / "drawing.svg"
    src.write_bytes(LC.TOOL_SVG)
    texts, streams = [], []
    for extra in ([], ["--hatch-connect"]):
        SV.main_stream([str(src), "--no-preview"] + LC.TOOL_ARGS + extra, **doubles(LC.HatchLinkDouble()))
        texts.append((tmp_path / "drawing.gcode").read_text()); streams.append((tmp_path / "drawing_stream.bin").read_bytes())
    assert texts[0] == texts[1] and streams[0] != streams[1] and pen_lifts(streams[1]) < pen_lifts(streams[0])
