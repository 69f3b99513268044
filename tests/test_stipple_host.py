"""--stipple-mm on the CPU: the sequential double of tests/stipple_double.py on the hand-checkable drawings of tests/stipple_cases.py; the option parsing
with every argument error and the lattice of `stagger`; and the whole front door of orip.svg run through the doubles: the taps of the stream are the
dots, each at its place and with its pen, --no-reorder plots the stated order, a drawing whose only ink is dots is not the empty stream, and without
the option the step is never called and the bytes are what they were.  No comparison has a tolerance."""
import numpy as np
import pytest

import stipple_cases as SC
import stipple_double as SD

CASES = SC.cases()


def run(name):
    return SD.stipple(*SC.args(CASES[name]))


def dots(xy):
    return [tuple(q) for q in np.asarray(xy).tolist()]


# ------------------------------------------------------------------ the double against the rule
def test_the_square_has_529_dots_row_after_row():
    xy, grp, st = run("square")
    want = [(x, y) for y in range(160, 1041, 40) for x in range(160, 1041, 40)]                  # 23 x 23: 27 inside the outline 100 .. 1100
    assert len(want) == 529 and dots(xy) == want and grp.tolist() == [0] * 529
    assert st == dict(groups=1, rows=26 - 1, candidates=625, near=96, outside=0, hidden=0, dots=529)
    assert dots(run("zero_length_edges")[0]) == want and run("zero_length_edges")[2] == st    # edges of zero length are ignored
    xy1, grp1, st1 = run("ring_of_one_point")                                                  # a shape of one point has no interior; a stray point widens a box only
    assert dots(xy1) == want and grp1.tolist() == [1] * 529 and st1["groups"] == 1 and st1["rows"] == 48


def test_points_on_the_outline_are_not_inside():
    got = set(dots(run("inset_0_vertex_on_lattice")[0]))                                       # the square 80 .. 400 on the lattice of 40, inset 0
    assert got == {(x, y) for x in range(120, 361, 40) for y in range(120, 361, 40)}           # no vertex, no point of an edge; their neighbours are dots
    got = set(dots(run("edge_on_row")[0]))
    assert (160, 240) in got and (120, 280) in got and (40, 360) in got                        # the ray of (160, 240) runs along the horizontal edge
    assert not {(200, 240), (240, 240), (400, 240), (160, 280), (80, 360), (0, 240), (40, 0), (400, 200)} & got      # vertex, horizontal edge, diagonal, sides
    assert all(0 < x < 400 and 0 < y and (y < 240 or x + y < 440) for x, y in got)
    got = set(dots(run("ray_through_vertex")[0]))                                              # the diamond's left and right vertices lie on the row y = 200
    assert {(x, 200) for x in range(40, 361, 40)} <= got and not {(0, 200), (400, 200), (200, 0), (200, 400), (100, 100), (-40, 200), (440, 200)} & got
    assert got == {(x, y) for x in range(0, 401, 40) for y in range(0, 401, 40) if abs(x - 200) + abs(y - 200) < 200}


def test_the_slit_and_the_rect():
    xy, _, st = run("slit")                                                                    # the slit is 20 wide: x = 590 .. 610 from y = 300 up
    assert all(not (563 < x < 637 and y > 273) for x, y in dots(xy)) and (560, 320) in dots(xy) and (640, 320) in dots(xy) and (600, 240) in dots(xy)
    xy, _, st = run("half_off_sheet")
    assert st["outside"] == 253 and st["dots"] == 276 == 12 * 23 and max(x for x, _ in dots(xy)) == 600
    assert run("no_rings")[2] == dict.fromkeys(SD.STATS, 0) and run("pitch_larger_than_shape")[0].tolist() == [[120, 120]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_identity_lattice_and_order(name):
    c = CASES[name]
    xy, grp, st = run(name)
    (p, q, s), (x0, y0, x1, y1) = c["lattice"], c["rect"]
    assert st["candidates"] == st["near"] + st["outside"] + st["hidden"] + st["dots"] and st["dots"] == len(xy) == len(grp)
    key = []
    for (x, y), g in zip(dots(xy), grp.tolist()):
        j = y // q
        assert y % q == 0 and (x - (s if j & 1 else 0)) % p == 0 and x0 <= x <= x1 and y0 <= y <= y1
        key.append((g, j, -x if c["flags"] & SD.SERPENTINE and j & 1 else x))
    assert key == sorted(key) and len(set(key)) == len(key)                                     # group, row, x; x descending in the odd rows under serpentine


def test_negative_rows_are_odd_by_their_last_bit():
    c = CASES["negative_rows"]
    xy, _, _ = run("negative_rows")
    rows = {}
    for x, y in dots(xy):
        rows.setdefault(y // 35, []).append(x)
    assert min(rows) < -50 and any(j & 1 for j in rows) and any(not j & 1 for j in rows)
    for j, xs in rows.items():
        assert xs == sorted(xs, reverse=bool(j & 1)) and all((x - (20 if j & 1 else 0)) % 40 == 0 for x in xs)
    moved, v = SC.shifted(c, 75, 86)                                                           # a lattice vector: the dots move with the drawing
    assert np.array_equal(SD.stipple(*SC.args(moved))[0], xy.astype(np.int64) + v)


def test_overlap_and_occlusion():
    plain, occ = run("overlap_3"), run("overlap_3_occlude")
    top = 900000000
    assert dots(plain[0][plain[1] == top]) == dots(occ[0][occ[1] == top])                       # the top shape loses nothing
    assert set(dots(occ[0])) <= set(dots(plain[0])) and occ[2]["hidden"] == plain[2]["dots"] - occ[2]["dots"] == 334
    both = set(dots(plain[0][plain[1] == 3])) & set(dots(plain[0][plain[1] == 7]))
    assert both and not both & set(dots(occ[0][occ[1] == 3]))                                   # a point of two shapes is a dot of each; the lower one's is hidden
    xy, grp, st = run("hole_on_top_occlude")                                                    # the hole of the upper shape hides nothing
    assert (600, 600) in dots(xy[grp == 0]) and (400, 400) not in dots(xy[grp == 0]) and (400, 400) in dots(xy[grp == 1]) and (600, 600) not in dots(xy[grp == 1])
    a, b, c = (run(f"near_diagonal_{k}")[2]["dots"] for k in "abc")
    assert (a, b, c) == (43, 18, 0)                                                             # one step of inset at 2^29: decided in the low bits of a 2^94 product
    for name in ("square", "gon_100", "l_shape"):                                               # raising the inset never adds a dot
        last = None
        for inset in (0, 5, 27, 28, 60):
            got = set(dots(SD.stipple(*SC.args(dict(CASES[name], inset=inset)))[0]))
            assert last is None or got <= last
            last = got


# ------------------------------------------------------------------ the options
def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def test_the_lattice_of_the_patterns():
    from orip import svg as SV
    assert SV.stipple_lattice(40, "square") == (40, 40, 0) and SV.stipple_lattice(40, "stagger") == (40, 35, 20)
    assert SV.stipple_lattice(2, "stagger") == (2, 2, 1) and SV.stipple_lattice(3, "stagger") == (3, 3, 1) and SV.stipple_lattice(7, "stagger") == (7, 6, 3)
    assert SV.stipple_lattice(1 << 20, "stagger") == (1 << 20, 908032, 1 << 19) and SV.stipple_lattice(1000, "stagger") == (1000, 866, 500)
    for p in (2, 3, 5, 40, 999, 1 << 20):
        _, q, s = SV.stipple_lattice(p, "stagger")
        assert 1 <= q <= 1 << 20 and 0 <= s < p
    assert SV.stipple_params(svg_options([])) is None
    assert SV.stipple_params(svg_options(["--stipple-mm", "1"])) == {"lattice": (40, 35, 20), "inset": 27}      # the hatch's default inset, 0.675 mm
    assert SV.stipple_params(svg_options(["--stipple-mm", "1.26", "--steps-per-mm", "10", "--stipple-pattern", "square", "--stipple-inset-mm", "0.25"])) == {"lattice": (13, 13, 0), "inset": 2}
    assert SV.stipple_params(svg_options(["--stipple-mm", "0.05", "--stipple-inset-mm", "0"])) == {"lattice": (2, 2, 1), "inset": 0}


@pytest.mark.parametrize("args", [["--stipple-inset-mm", "1"], ["--stipple-pattern", "square"], ["--stipple-mm", "0"], ["--stipple-mm", "-1"], ["--stipple-mm", "nan"],
                                  ["--stipple-mm", "inf"], ["--stipple-mm", "0.03"], ["--stipple-mm", "26215"], ["--stipple-mm", "1e300"],
                                  ["--stipple-mm", "1", "--stipple-inset-mm", "-0.1"], ["--stipple-mm", "1", "--stipple-inset-mm", "nan"],
                                  ["--stipple-mm", "1", "--stipple-inset-mm", "26215"]])
def test_argument_errors_end_the_run_before_any_device_step(args, tmp_path):
    from orip import svg as SV

    def never(*a, **k):
        raise AssertionError("a device step ran")
    with pytest.raises(ValueError, match="stipple"):
        SV.stipple_params(svg_options(args))
    (tmp_path / "in.svg").write_bytes(SC.TOOL_SVG)
    with pytest.raises(ValueError, match="stipple"):
        SV.main_stream([str(tmp_path / "in.svg"), "--no-preview"] + args, flatten_fn=never, bbox_fn=never, fit_fn=never, fetch_fn=never, stipple_fn=never)
    with pytest.raises(SystemExit):
        SV.build_stream_argparser().parse_args(["in.svg", "--stipple-mm", "1", "--stipple-pattern", "hexagonal"])
    with pytest.raises(SystemExit):
        SV.build_gcode_argparser().parse_args(["in.svg", "--stipple-mm", "1"])                  # svg2gcode.py does not get the option: G-code has no tap


# ------------------------------------------------------------------ the whole front door through the doubles
def doubles(stipple=None, **more):
    import clip_double as CD
    import dedup_double as DD
    import occlude_cases as OC
    import seam_double as SM
    import simplify_double as SP

    return dict(dict(CD.svg_doubles(), dedup_fn=DD.dedup_numpy, occlude_fn=OC.OccludeDouble(), seam_fn=SM.seams, simplify_fn=SP.simplify_numpy, stipple_fn=stipple), **more)


def taps_of(data):
    """the taps of a stream, in order: [(colour, (x, y))]"""
    import stream_preview_double as SPD
    _, kind, val = SPD.decode(data)
    x = y = col = 0
    out = []
    for k, v in zip(kind.tolist(), val.tolist()):
        if k == SPD.K_STEP:
            x += int(SPD.DX[v]); y += int(SPD.DY[v])
        elif k == SPD.K_COLOR:
            col = v
        elif k == SPD.K_PEN and v == 3:
            out.append((col, (x, y)))
    return out


STIPPLE = ["--stipple-mm", "4", "--stipple-inset-mm", "1.5"]


def test_without_the_option_nothing_changes_and_the_step_is_never_called():
    from orip import svg as SV
    Z = SC.StippleDouble()
    for extra in ([], ["--pen-colors", "#00f,#f00", "--allow-reverse"], ["--hatch-spacing-mm", "4", "--occlude", "--loop-start"]):
        a = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(SC.TOOL_ARGS + extra), **doubles())
        b = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(SC.TOOL_ARGS + extra), **doubles(Z))
        assert a[0] == b[0] and Z.calls == 0 and "stipple" not in b[1] and "taps" not in b[1] and not taps_of(b[0])


def test_the_taps_of_the_stream_are_the_dots():
    from orip import svg as SV
    import merge_cases as MC
    Z = SC.StippleDouble()
    plain, pinfo = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(SC.TOOL_ARGS), **doubles())
    data, info = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(SC.TOOL_ARGS + STIPPLE), **doubles(Z))
    xy, grp, st = Z.out
    assert Z.calls == 1 and Z.args["lattice"] == (40, 35, 20) and Z.args["inset"] == 15 and Z.args["rect"] == (0, 0, 2099, 2969) and Z.args["flags"] == SD.SERPENTINE
    assert Z.args["clamp"] and Z.args["ring_group"].tolist() == [0, 2] and len(Z.args["ring_off"]) == 3            # the two filled rectangles; the circle has no fill
    assert {k: info["stipple"][k] for k in SD.STATS} == st and info["taps"] == st["dots"] == len(xy) > 100 and sorted(set(grp.tolist())) == [0, 2]
    taps = taps_of(data)
    assert len(taps) == st["dots"] and sorted(t[1] for t in taps) == sorted(dots(xy)) and {t[0] for t in taps} == {3}      # each tap at its dot, --color-index
    assert MC.strokes_of(data) and len(MC.strokes_of(data)) == len(MC.strokes_of(plain)) and info["paths"] == pinfo["paths"]      # the strokes are all there
    line = [ln for ln in __import__("orip.gcode", fromlist=["x"]).report_lines("svg", info) if "stipple" in ln]
    assert line == [f"[svg] stipple: {st['dots']} dots in 2 shapes (pitch 40, rows 35; {st['near']} near the outline, 0 off the sheet, 0 hidden)"]


def test_no_reorder_plots_the_stated_order_and_the_pens_are_the_shapes():
    from orip import svg as SV
    Z = SC.StippleDouble()
    data, info = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(SC.TOOL_ARGS + STIPPLE + ["--no-reorder", "--stipple-pattern", "square"]), **doubles(Z))
    assert [t[1] for t in taps_of(data)] == dots(Z.out[0]) and Z.args["lattice"] == (40, 40, 0)                     # group, row, x; serpentine
    plain = SC.StippleDouble()
    SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(SC.TOOL_ARGS + STIPPLE + ["--no-reorder", "--no-serpentine"]), **doubles(plain))
    assert plain.args["flags"] == 0 and sorted(dots(plain.out[0])) != dots(plain.out[0])
    Z = SC.StippleDouble()
    data, info = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(SC.TOOL_ARGS + STIPPLE + ["--pen-colors", "#00f,#f00,#000", "--occlude", "--clip", "--improve-order"]), **doubles(Z))
    xy, grp, st = Z.out
    assert Z.args["flags"] == SD.SERPENTINE | SD.OCCLUDE and not Z.args["clamp"] and st["hidden"] > 0
    pen_of = {0: 0, 2: 1}                                                                       # the blue fill takes the blue pen, the red fill the red one
    assert sorted(taps_of(data)) == sorted((pen_of[g], p) for p, g in zip(dots(xy), grp.tolist()))
    assert info["pens"]["paths"][0] == 1 + int((grp == 0).sum()) and info["pens"]["paths"][1] == 1 + int((grp == 2).sum()) and info["pens"]["paths"][2] == 1


def test_loop_start_sees_a_dot_as_the_open_stroke_p_p():
    from orip import svg as SV
    import seam_double as SM
    seen = []

    def seam_fn(off, pts, order, rev):
        seen.append((np.asarray(off).copy(), np.asarray(pts).copy()))
        return SM.seams(off, pts, order, rev)
    Z = SC.StippleDouble()
    data, info = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(SC.TOOL_ARGS + STIPPLE + ["--loop-start"]), **doubles(Z, seam_fn=seam_fn))
    off, pts = seen[0]
    D = Z.out[2]["dots"]
    tail = pts[off[-1 - D]:].reshape(D, 2, 2)
    assert (np.diff(off) >= 2).all() and (np.diff(off)[-D:] == 2).all() and np.array_equal(tail[:, 0], tail[:, 1]) and np.array_equal(tail[:, 0], Z.out[0])
    assert info["seam"]["closed"] == 3 and len(taps_of(data)) == D


def test_a_drawing_whose_only_ink_is_dots_is_not_the_empty_stream():
    from orip import gcode as GC, svg as SV
    import dash_double as DD
    gap = SC.TOOL_SVG_DOTS_ONLY.replace(b'stroke="#00f"', b'stroke="#00f" stroke-dasharray="1 2000" stroke-dashoffset="2"')      # the whole outline lies in the gap
    none, _ = SV.build_stream_from_svg(gap, svg_options(SC.TOOL_ARGS + ["--dashes"]), **doubles(dash_fn=DD.dash_numpy))
    assert none == GC.EMPTY_STREAM
    for extra in ([], ["--pen-colors", "#00f,#f00"], ["--loop-start", "--allow-reverse"]):
        Z = SC.StippleDouble()
        data, info = SV.build_stream_from_svg(gap, svg_options(SC.TOOL_ARGS + ["--dashes"] + STIPPLE + extra), **doubles(Z, dash_fn=DD.dash_numpy))
        assert data != GC.EMPTY_STREAM and info["paths"] == 0 and info["taps"] == Z.out[2]["dots"] > 0
        assert sorted(t[1] for t in taps_of(data)) == sorted(dots(Z.out[0])) and {t[0] for t in taps_of(data)} == ({0} if "--pen-colors" in extra else {3})
    narrow = SC.TOOL_SVG_DOTS_ONLY.replace(b'width="100" height="100"', b'width="2" height="2"')                  # and a drawing with neither ends as it always did
    data, info = SV.build_stream_from_svg(narrow.replace(b'stroke="#00f"', b'stroke="#00f" stroke-dasharray="1 2000" stroke-dashoffset="2"'),
                                          svg_options(SC.TOOL_ARGS + ["--dashes"] + STIPPLE), **doubles(SC.StippleDouble(), dash_fn=DD.dash_numpy))
    assert data == GC.EMPTY_STREAM and info["taps"] == 0
