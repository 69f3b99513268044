"""--simplify-mm on the host, without a GPU: the sequential double (tests/simplify_double.py) gives the hand-worked answers of the rule; on random strokes the
invariants hold that need no second opinion (a subsequence with both ends, every dropped point within the tolerance of the kept segment that spans it, a
second pass changes nothing, tolerance 0 without collinear triples changes nothing); and the host flow of both tools with every device step injected as a
double: the option parses, without it nothing is called and every byte is what it was, with it pieces and bytes go down and the strokes stay, and it
composes with --merge-paths, --clip, pens and --improve-order.  No comparison here has a tolerance."""
import numpy as np
import pytest

import clip_double as CD
import gcode_double as D
import merge_cases as MC
import pens_double as PD
import simplify_cases as SC
import simplify_double as SD
from stream_double import codes_numpy


def never(*a, **k):
    raise AssertionError("the simplification was called without --simplify-mm")


NP = SC.LINE_STROKES + SC.CURVES                # strokes of the tool drawing; the plain two-point line of every copy cannot change
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)


class Simplify:
    """simplify_double.simplify_numpy that remembers what it was given and what it returned"""
    def __init__(self): self.calls = []

    def __call__(self, off, pts, tol4):
        out = SD.simplify_numpy(off, pts, tol4)
        self.calls.append(((np.array(off), np.array(pts), tol4), out))
        return out


# ------------------------------------------------------------------ the rule, on the double
@pytest.mark.parametrize("k", range(len(SC.HAND)))
def test_hand_worked(k):
    pts, tol4, kept = SC.HAND[k]
    assert SD.simplify_stroke(pts, tol4) == kept


def test_staircase():
    for tol4, count in SC.STAIR_COUNTS.items():
        kept = SD.simplify_stroke(SC.staircase(), tol4)
        assert len(kept) == count, tol4
    assert SD.simplify_stroke(SC.staircase(), 3) == [0, 200]


def test_the_crafted_products_need_128_bits():
    A, B, P, Q = SC.cross_pair()
    assert SD.simplify_stroke([A, P, Q, B], 8) == [0, 2, 3] and SD.simplify_stroke([A, Q, P, B], 8) == [0, 1, 3]      # Q, whose product is larger by one
    kP, kQ = SD.key(A, B, P)[0], SD.key(A, B, Q)[0]
    assert kQ > kP and float(kQ) == float(kP) and (kQ >> 64) == (kP >> 64)        # a double or the upper word alone cannot tell them apart
    for which, kept in (("below", [0, 2]), ("above", [0, 1, 2])):
        pts, tol4 = SC.near_threshold(which)
        assert SD.simplify_stroke(pts, tol4) == kept
        K, L = SD.key(pts[0], pts[2], pts[1])
        assert float(16 * K) == float(tol4 * tol4 * L)


def random_strokes(seed, n=40, collinear=True):
    rng = np.random.default_rng(seed)
    lists = []
    for _ in range(n):
        k = int(rng.integers(2, 60))
        if collinear:                                                         # a small box: many collinear triples, many ties
            P = rng.integers(0, 12, (k, 2))
        else:                                                                 # x strictly increasing and y on a parabola with noise in the high bits: no three points on a line
            x = np.cumsum(rng.integers(1, 5, k))
            P = np.stack([x, x * x + 1], 1)
        keep = np.ones(k, bool); keep[1:] = (np.diff(P, axis=0) != 0).any(1)
        P = P[keep]
        if len(P) >= 2:
            lists.append([tuple(q) for q in P.tolist()])
    return SC.strokes(lists)


@pytest.mark.parametrize("tol4", [0, 1, 4, 9, 40])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_invariants(seed, tol4):
    off, pts = random_strokes(seed)
    o2, p2, kept, st = SD.simplify_numpy(off, pts, tol4)
    n = len(off) - 1
    assert len(o2) == n + 1 and st == {"paths": n, "points_in": len(pts), "points_out": len(kept), "rounds": 0}
    assert np.array_equal(kept[o2[:-1]], off[:-1]) and np.array_equal(kept[o2[1:] - 1], off[1:] - 1) and (np.diff(kept) > 0).all()      # a subsequence with both ends
    assert np.array_equal(p2, pts[kept]) and not (np.diff(p2, axis=0)[np.delete(np.arange(len(p2) - 1), o2[1:-1] - 1)] == 0).all(1).any()
    flat = [tuple(q) for q in pts.tolist()]
    for a, b in zip(kept[:-1].tolist(), kept[1:].tolist()):                   # every dropped point against its kept neighbours
        for i in range(a + 1, b):
            assert SD.within(flat[a], flat[b], flat[i], tol4), (a, i, b)
    again = SD.simplify_numpy(o2, p2, tol4)
    assert np.array_equal(again[0], o2) and np.array_equal(again[1], p2) and np.array_equal(again[2], np.arange(len(p2)))      # idempotent
    if tol4:
        assert st["points_out"] < st["points_in"]


def test_tolerance_zero_without_collinear_triples_changes_nothing():
    off, pts = random_strokes(7, collinear=False)
    o2, p2, kept, st = SD.simplify_numpy(off, pts, 0)
    assert np.array_equal(o2, off) and np.array_equal(p2, pts) and np.array_equal(kept, np.arange(len(pts)))


def test_two_point_strokes_pass_through():
    off, pts, tol4 = SC.cases()["two_points_only"]
    o2, p2, kept, st = SD.simplify_numpy(off, pts, tol4)
    assert np.array_equal(o2, off) and np.array_equal(p2, pts) and st["points_out"] == 6
    o2, p2, kept, st = SD.simplify_numpy([0], np.zeros((0, 2)), 5)
    assert o2.tolist() == [0] and p2.shape == (0, 2) and len(kept) == 0 and st["paths"] == 0


def test_the_double_refuses_what_the_device_refuses():
    ok = ([0, 3], [[1, 1], [2, 2], [3, 1]])
    SD.simplify_numpy(*ok, 0)
    for off, pts, tol4 in ((ok[0], ok[1], -1), (ok[0], ok[1], 1 << 17), ([1, 3], ok[1], 0), ([0, 1, 3], ok[1], 0), ([0, 3], [[1, 1], [1, 1], [3, 1]], 0),
                           ([0, 3], [[1, 1], [-2, 2], [3, 1]], 0), ([0, 3], [[1, 1], [2, 2], [3, (1 << 30) + 1]], 0), ([0, 2], ok[1], 0)):
        with pytest.raises(ValueError):
            SD.simplify_numpy(off, pts, tol4)
    SD.simplify_numpy([0, 2, 4], [[1, 1], [2, 2], [2, 2], [3, 1]], 0)          # the end of one stroke may be the start of the next


# ------------------------------------------------------------------ the command lines
def test_option_parses_on_both_tools():
    from orip import svg as SV, gcode as GC
    assert GC.GcodeOptions().simplify_mm is None and SV.SvgOptions().simplify_mm is None
    assert GC.build_argparser().parse_args(["in.gcode"]).simplify_mm is None and SV.build_stream_argparser().parse_args(["in.svg"]).simplify_mm is None
    assert GC.options_from_args(GC.build_argparser().parse_args(["in.gcode", "--simplify-mm", "0"])).simplify_mm == 0.0
    o = SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--simplify-mm", "0.05"]))
    assert o.simplify_mm == 0.05 and SV.gcode_options(o).simplify_mm == 0.05 and SV.gcode_options(SV.SvgOptions()).simplify_mm is None
    assert not hasattr(SV.build_gcode_argparser().parse_args(["in.svg"]), "simplify_mm")       # svg2gcode.py writes G-code: the pass lives in the stream


def test_tolerance_in_quarter_steps():
    from orip import gcode as GC
    t = lambda mm, spm=40.0: GC.simplify_tol4(GC.GcodeOptions(simplify_mm=mm, steps_per_mm=spm))
    assert t(None) is None and t(0) == 0 and t(0.025) == 4 and t(0.1) == 16 and t(0.003) == 0 and t(0.004) == 1 and t(1.0, 80.0) == 320
    assert t(819.0) == 131040 and t(((1 << 17) - 1) / 160.0) == (1 << 17) - 1
    for mm, spm in ((-0.1, 40.0), (float("nan"), 40.0), (float("inf"), 40.0), (820.0, 40.0), (1 << 17, 0.25), (1e300, 40.0)):
        with pytest.raises(ValueError):
            t(mm, spm)


def test_option_errors_come_before_any_step():
    from orip import gcode as GC, svg as SV
    text = SC.tool_gcode()
    dead = {k: never for k in ("steps_fn", "order_fn", "codes_fn", "pack_fn", "simplify_fn")}
    for mm in (-1.0, float("nan"), 1e9):
        with pytest.raises(ValueError):
            GC.build_stream_from_gcode(text, GC.GcodeOptions(simplify_mm=mm), **dead)
        with pytest.raises(ValueError):
            SV.build_stream_from_svg(SC.tool_svg(), SV.SvgOptions(simplify_mm=mm), **dict(PD.pens_doubles(), simplify_fn=never, steps_fn=never))
    # a result that is not the same strokes thinned is refused
    wrong = [lambda off, pts, t: (off, pts[::-1].copy(), np.arange(len(pts)), {}), lambda off, pts, t: (off[:-1], pts[:off[-2]], np.arange(off[-2]), {}),
             lambda off, pts, t: (np.array([0, 2] + (off[2:] - off[1] + 2).tolist()), pts[np.r_[0, 1, off[1]:len(pts)]], np.r_[0, 1, off[1]:len(pts)], {})]
    for fn in wrong:
        with pytest.raises(RuntimeError):
            GC.build_stream_from_gcode(text, GC.GcodeOptions(simplify_mm=0.1), simplify_fn=fn, **GCODE_DOUBLES)


# ------------------------------------------------------------------ the host flow through the doubles
def test_off_by_default_and_bytes_unchanged():
    from orip import gcode as GC, svg as SV
    from test_gcode_host import G, MAIN_CASES, options_for
    for i, (name, args) in enumerate(MAIN_CASES):
        data, info = GC.build_stream_from_gcode(bytes(G[f"text_{name}"]), options_for(args), simplify_fn=never, **GCODE_DOUBLES)
        assert data == bytes(G[f"main_{i}_bin"]) and "simplify" not in info
    text = SC.tool_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(), **GCODE_DOUBLES)
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(simplify_mm=None), simplify_fn=never, **GCODE_DOUBLES)
    assert data == plain and info == pinfo
    o = SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview", "--pen-colors", "#f00,#00f"]))
    a = SV.build_stream_from_svg(SC.tool_svg(), o, **PD.pens_doubles())
    b = SV.build_stream_from_svg(SC.tool_svg(), o, simplify_fn=never, **PD.pens_doubles())
    assert a[0] == b[0] and "simplify" not in b[1]


def test_gcode_flow_thins_the_strokes_before_the_order():
    from orip import gcode as GC
    text = SC.tool_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(), **GCODE_DOUBLES)
    Z = Simplify()
    tm = {}
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(simplify_mm=SC.TOOL_MM), simplify_fn=Z, timings=tm, **GCODE_DOUBLES)
    (off, pts, tol4), out = Z.calls[0]
    assert len(Z.calls) == 1 and tol4 == 16 and "simplify" in tm and len(off) - 1 == pinfo["paths"] == NP
    st = info["simplify"]
    assert st == {"tol4": 16, "points_in": len(pts), "points_out": len(out[1]), "paths_changed": NP - SC.COPIES} and st["points_out"] * 4 < st["points_in"]
    assert info["paths"] == pinfo["paths"] and info["pieces"] < pinfo["pieces"] and info["bytes"] < pinfo["bytes"] and len(data) < len(plain)
    assert info["moves"] == pinfo["moves"] - (st["points_in"] - st["points_out"])
    got, was = MC.strokes_of(data), MC.strokes_of(plain)
    assert len(got) == len(was) == NP and sorted((s[0], s[-1]) for _, s in got) == sorted((s[0], s[-1]) for _, s in was)       # the same strokes between the same ends
    # tolerance 0 on the lines alone: only the vertices on the lines go, and the pen draws the same steps
    lines = SC.tool_gcode(curves=False)
    p0, i0 = GC.build_stream_from_gcode(lines, GC.GcodeOptions(), **GCODE_DOUBLES)
    d0, j0 = GC.build_stream_from_gcode(lines, GC.GcodeOptions(simplify_mm=0.0), simplify_fn=Simplify(), **GCODE_DOUBLES)
    assert j0["simplify"]["tol4"] == 0 and j0["simplify"]["points_out"] == SC.LINE_CORNERS and j0["simplify"]["paths_changed"] == 3 * SC.COPIES
    assert j0["pieces"] < i0["pieces"] and j0["bytes"] < i0["bytes"] and j0["steps"] == i0["steps"]
    assert [s for _, s in MC.strokes_of(d0)] == [s for _, s in MC.strokes_of(p0)]


def test_gcode_flow_with_the_other_options():
    """after the merge (the joints of a merged chain go), with the clip's strokes, with pens (a stroke keeps its pen) and before the order's improvement"""
    from orip import gcode as GC
    text = MC.tool_gcode()                                                    # the sine exploded into 299 strokes, a square and a triangle stroke by stroke
    Z = Simplify()
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(merge_paths=True, simplify_mm=0.05), **dict(CD.gcode_doubles(), simplify_fn=Z))
    (off, pts, tol4), out = Z.calls[0]
    assert info["merge"]["paths_out"] == 5 == len(off) - 1 == info["paths"] and tol4 == 8
    assert info["simplify"]["points_in"] == len(pts) > 300 and info["simplify"]["points_out"] < 120 and info["simplify"]["paths_changed"] >= 1
    alone, ainfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(simplify_mm=0.05), **dict(CD.gcode_doubles(), simplify_fn=Simplify()))
    assert ainfo["simplify"]["paths_changed"] == 0 and ainfo["simplify"]["points_in"] == ainfo["simplify"]["points_out"] == 2 * 307       # two-point strokes pass through
    lines = ["G21 G90 M5"]
    paths = [(1, [(20, 20), (-10, 30), (20, 40), (-10, 50), (20, 60)]), (2, [(30, 100), (10, 100), (-20, 100)]), (1, [(50, 50), (55, 55), (60, 60)]), (2, [(0, 100), (0, 150), (40, 150)])]
    for t, s in paths:
        lines += ["T%d" % t, "G0 X%g Y%g" % s[0], "M3"] + ["G1 X%g Y%g" % q for q in s[1:]] + ["M5"]
    text = "\n".join(lines) + "\n"
    base = dict(clip=True, tool_pens=True, simplify_mm=0.0)
    Z = Simplify()
    d1, i1 = GC.build_stream_from_gcode(text, GC.GcodeOptions(**base), **dict(CD.gcode_doubles(), steps_fn=never, simplify_fn=Z))
    assert i1["clip"]["paths_out"] == i1["paths"] == len(Z.calls[0][0][0]) - 1 and i1["simplify"]["paths_changed"] == 2 and i1["pens"]["paths"][:3] == [0, 4, 2]
    d2, i2 = GC.build_stream_from_gcode(text, GC.GcodeOptions(allow_reverse=True, improve_order=True, merge_paths=True, **base), **dict(CD.gcode_doubles(), steps_fn=never, simplify_fn=Simplify()))
    assert i2["merge"]["joins"] == 1 and i2["simplify"]["points_in"] == i1["simplify"]["points_in"] - 1 and i2["improve"]["travel_after"] <= i2["improve"]["travel_before"]
    plain, _ = GC.build_stream_from_gcode(text, GC.GcodeOptions(clip=True, tool_pens=True), **dict(CD.gcode_doubles(), steps_fn=never))
    down = lambda d: sum(len(s) - 1 for _, s in MC.strokes_of(d))
    assert down(d1) == down(d2) == down(plain) and sorted(c for c, _ in MC.strokes_of(d1)) == sorted(c for c, _ in MC.strokes_of(plain))


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def test_svg_flow_forwards_the_option():
    from orip import svg as SV
    plain, pinfo = SV.build_stream_from_svg(SC.tool_svg(), svg_options(SC.TOOL_SVG_ARGS[2:]), want_paths=True, **PD.pens_doubles())
    Z = Simplify()
    data, info = SV.build_stream_from_svg(SC.tool_svg(), svg_options(SC.TOOL_SVG_ARGS), want_paths=True, **dict(PD.pens_doubles(), simplify_fn=Z))
    assert len(Z.calls) == 1 and Z.calls[0][0][2] == 16 and info["simplify"]["tol4"] == 16 and info["simplify"]["points_out"] * 4 < info["simplify"]["points_in"]
    assert info["paths"] == pinfo["paths"] == NP and info["pieces"] < pinfo["pieces"] and info["bytes"] < pinfo["bytes"] and info["pens"] == pinfo["pens"]
    assert np.array_equal(info["fitted_paths"][1], pinfo["fitted_paths"][1])                   # the G-code file does not know of the pass
    assert [c for c, _ in MC.strokes_of(data)] == [c for c, _ in MC.strokes_of(plain)]
    d2, i2 = SV.build_stream_from_svg(SC.tool_svg(), svg_options(SC.TOOL_SVG_ARGS + ["--merge-paths", "--allow-reverse", "--improve-order", "--clip"]),
                                      **dict(CD.svg_doubles(), steps_fn=never, simplify_fn=Simplify()))
    assert i2["simplify"]["points_out"] == info["simplify"]["points_out"] and i2["merge"]["joins"] == 0 and i2["clip"]["cut"] == 0


def test_the_tools_print_the_simplify_line(tmp_path, capsys):
    from orip import gcode as GC, svg as SV
    (tmp_path / "c.gcode").write_text(SC.tool_gcode())
    GC.main([str(tmp_path / "c.gcode"), "-o", str(tmp_path / "c.bin"), "--simplify-mm", "0.1"], **dict(GCODE_DOUBLES, simplify_fn=SD.simplify_numpy))
    out = capsys.readouterr().out
    want = SD.simplify_numpy(*D.to_steps_numpy(*__import__("orip.gcode", fromlist=["x"]).parse_gcode(SC.tool_gcode())[:2], MAP40), 16)[3]
    assert f"[gcode] simplify: {want['points_in']} points -> {want['points_out']} within 4 steps, {NP - SC.COPIES} strokes changed" in out
    (tmp_path / "d.svg").write_bytes(SC.tool_svg())
    SV.main_stream([str(tmp_path / "d.svg"), "--no-preview"] + SC.TOOL_SVG_ARGS, **dict(PD.pens_doubles(), simplify_fn=SD.simplify_numpy))
    out = capsys.readouterr().out
    assert "[svg] simplify: " in out and " within 4 steps, " in out and (tmp_path / "d_stream.bin").exists()
    GC.main([str(tmp_path / "c.gcode"), "-o", str(tmp_path / "c.bin"), "--simplify-mm", "0.03"], **dict(GCODE_DOUBLES, simplify_fn=SD.simplify_numpy))
    assert " within 1.25 steps, " in capsys.readouterr().out


MAP40 = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=40.0, W=8400, H=11880, invert_y=0)
