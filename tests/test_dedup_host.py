"""--dedup on the host, without a GPU: the sequential double (tests/dedup_double.py) gives the hand-worked answers of the rule; on seeded random drawings and on
the named ones the consequences hold that need no second opinion (the output's primitive steps are the support of the input's, each once; a drawing without a
shared step comes back unchanged; a second pass changes nothing; strokes of two points or more without repeats whose interior vertices are input vertices;
pieces <= 2 segments); and the host flow of both tools with every device step injected as a double: the option parses, without it nothing is called and
every byte is what it was, with it and --merge-paths the grid of squares is drawn with fewer pen lifts than it has squares, and a return that does not hold
is refused.  No comparison here has a tolerance."""
import numpy as np
import pytest

import dedup_cases as DC
import dedup_double as DD
import gcode_double as D
import merge_double as MD
import pens_double as PD
from stream_double import codes_numpy

CASES = DC.cases()
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)


def never(*a, **k):
    raise AssertionError("the dedup was called without --dedup")


class Dedup:
    """dedup_double.dedup_numpy that remembers what it was given and what it returned"""
    def __init__(self): self.calls = []

    def __call__(self, off, pts, group, n_groups):
        out = DD.dedup_numpy(off, pts, group, n_groups)
        self.calls.append(((np.array(off), np.array(pts), np.array(group), n_groups), out))
        return out


# ------------------------------------------------------------------ the rule, on the double
@pytest.mark.parametrize("k", range(len(DC.HAND)))
def test_hand_worked(k):
    lists, groups, want, origin = DC.HAND[k]
    out, org, st = DD.dedup_lists(lists, groups)
    assert [[tuple(q) for q in s] for s in out] == want and org == origin
    assert st["paths_out"] == len(want) and st["points_out"] == sum(len(s) for s in want) and st["whole"] + st["cut"] + st["covered"] == st["segments"]


def test_the_grid_saves_its_inner_edges():
    off, pts, group, n_groups = CASES["grid_3x3"]
    st = DD.dedup_numpy(off, pts, group, n_groups)[3]
    assert (st["draw_steps_in"], st["draw_steps_out"], st["covered"], st["cut"]) == (36 * DC.L, 24 * DC.L, 12, 0)      # 12 inner edges, each in the file twice


def consequences(off, pts, group, n_groups, expand=True):
    o2, p2, origin, st = DD.dedup_numpy(off, pts, group, n_groups)
    n, k = len(off) - 1, len(o2) - 1
    g = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)
    assert (np.diff(origin) >= 0).all() and origin[0] >= 0 and origin[-1] < n and len(origin) == k
    if expand:                                                                # 1: a set, equal to the support of the input's multiset
        was, now = DD.primitive_steps(off, pts, g), DD.primitive_steps(o2, p2, g[origin])
        assert set(now.values()) == {1} and set(now) == set(was)
        if set(was.values()) == {1}:                                          # 2: nothing shared, nothing changed
            assert np.array_equal(o2, off) and np.array_equal(p2, pts) and np.array_equal(origin, np.arange(n))
    again = DD.dedup_numpy(o2, p2, g[origin], n_groups)                       # 3: idempotent
    assert np.array_equal(again[0], o2) and np.array_equal(again[1], p2) and np.array_equal(again[2], np.arange(k)) and again[3]["whole"] == again[3]["segments"] == st["pieces"]
    assert (np.diff(o2) >= 2).all() and not np.delete((np.diff(p2, axis=0) == 0).all(1), o2[1:-1] - 1).any()      # 4
    for j, (a, b) in enumerate(zip(o2[:-1].tolist(), o2[1:].tolist())):
        s = int(origin[j])
        own = {tuple(q) for q in pts[off[s]:off[s + 1]].tolist()}
        assert all(tuple(q) in own for q in p2[a + 1:b - 1].tolist())         # a cut point only ever begins or ends a stroke
    assert st["pieces"] <= 2 * st["segments"] and st["points_out"] <= 4 * st["segments"] and st["points_out"] == st["pieces"] + st["paths_out"]      # 5
    assert st["whole"] + st["cut"] + st["covered"] == st["segments"] == len(pts) - n and st["draw_steps_out"] <= st["draw_steps_in"]
    return st


def test_consequences_on_random_drawings():
    overlaps = 0
    for seed in range(1500):
        st = consequences(*DC.random_drawing(seed))
        overlaps += st["draw_steps_out"] < st["draw_steps_in"]
    assert 300 < overlaps < 1200                                              # both kinds are there


@pytest.mark.parametrize("name", sorted(CASES))
def test_consequences_on_the_named_drawings(name):
    off, pts, group, n_groups = CASES[name]
    far = int(np.abs(np.diff(pts.astype(np.int64), axis=0)).max()) > 1 << 20  # segments of 2^29 steps are not expanded step by step
    consequences(off, pts, group, n_groups, expand=not far)


def test_the_drawn_set_does_not_depend_on_direction():
    for seed in range(200):
        off, pts, group, n_groups = DC.random_drawing(seed)
        rev = np.concatenate([pts[a:b][::-1] for a, b in zip(off[:-1], off[1:])])
        a, b = DD.dedup_numpy(off, pts, group, n_groups), DD.dedup_numpy(off, rev, group, n_groups)
        assert set(DD.primitive_steps(a[0], a[1], group[a[2]])) == set(DD.primitive_steps(b[0], b[1], group[b[2]]))


def test_the_double_refuses_what_the_device_refuses():
    ok = ([0, 3], [[1, 1], [2, 2], [3, 1]])
    DD.dedup_numpy(*ok)
    for off, pts, group, n_groups in ((([1, 3]), ok[1], None, 1), ([0, 1, 3], ok[1], None, 1), ([0, 3], [[1, 1], [1, 1], [3, 1]], None, 1), ([0, 3], [[1, 1], [-2, 2], [3, 1]], None, 1),
                                      ([0, 3], [[1, 1], [2, 2], [3, (1 << 30) + 1]], None, 1), ([0, 2], ok[1], None, 1), (ok[0], ok[1], [1], 1), (ok[0], ok[1], [0], 65), (ok[0], ok[1], [0, 0], 1)):
        with pytest.raises(ValueError):
            DD.dedup_numpy(off, pts, group, n_groups)
    DD.dedup_numpy([0, 2, 4], [[1, 1], [2, 2], [2, 2], [3, 1]])               # the end of one stroke may be the start of the next


# ------------------------------------------------------------------ the command lines
def test_option_parses_on_both_tools():
    from orip import svg as SV, gcode as GC
    assert GC.GcodeOptions().dedup is False and SV.SvgOptions().dedup is False
    assert GC.build_argparser().parse_args(["in.gcode"]).dedup is False and SV.build_stream_argparser().parse_args(["in.svg"]).dedup is False
    assert GC.options_from_args(GC.build_argparser().parse_args(["in.gcode", "--dedup"])).dedup is True
    assert GC.options_from_args(GC.build_argparser().parse_args(["in.gcode", "--dedup", "--no-reorder"])).no_reorder is True       # strokes keep file order
    o = SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--dedup"]))
    assert o.dedup is True and SV.gcode_options(o).dedup is True and SV.gcode_options(SV.SvgOptions()).dedup is False
    assert not hasattr(SV.build_gcode_argparser().parse_args(["in.svg"]), "dedup")           # svg2gcode.py writes G-code: the pass lives in the stream
    import recording_device as RD
    gcode_steps, svg_steps = RD.doors_take_the_pass_table()
    assert GC.STROKE_ARGS[-1] == "--dedup" and "dedup_fn" in gcode_steps and "dedup_fn" in svg_steps and GC.StrokeSteps({}).fn.get("dedup") is None


# ------------------------------------------------------------------ the host flow through the doubles
def test_off_by_default_and_bytes_unchanged():
    from orip import gcode as GC, svg as SV
    from test_gcode_host import G, MAIN_CASES, options_for
    for i, (name, args) in enumerate(MAIN_CASES):
        data, info = GC.build_stream_from_gcode(bytes(G[f"text_{name}"]), options_for(args), dedup_fn=never, **GCODE_DOUBLES)
        assert data == bytes(G[f"main_{i}_bin"]) and "dedup" not in info
    text = DC.tool_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(), **GCODE_DOUBLES)
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(dedup=False), dedup_fn=never, **GCODE_DOUBLES)
    assert data == plain and info == pinfo
    o = SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview", "--pen-colors", "#f00,#00f"]))
    a = SV.build_stream_from_svg(DC.tool_svg(), o, **PD.pens_doubles())
    b = SV.build_stream_from_svg(DC.tool_svg(), o, dedup_fn=never, **PD.pens_doubles())
    assert a[0] == b[0] and "dedup" not in b[1]


def down_steps(data):
    import merge_cases as MC
    return sum(max(abs(q[0] - p[0]), abs(q[1] - p[1])) for _, s in MC.strokes_of(data) for p, q in zip(s[:-1], s[1:]))


def test_gcode_flow_draws_the_grid_once():
    from orip import gcode as GC
    import merge_cases as MC
    text = DC.tool_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(), **GCODE_DOUBLES)
    Z, tm = Dedup(), {}
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(dedup=True), dedup_fn=Z, timings=tm, **GCODE_DOUBLES)
    (off, pts, group, n_groups), out = Z.calls[0]
    assert len(Z.calls) == 1 and "dedup" in tm and len(off) - 1 == pinfo["paths"] == 9 and n_groups == 1 and not group.any()
    assert info["dedup"] == out[3] and (info["dedup"]["draw_steps_in"], info["dedup"]["draw_steps_out"]) == (DC.GRID_STEPS_IN, DC.GRID_STEPS_OUT)
    assert down_steps(plain) == DC.GRID_STEPS_IN and down_steps(data) == DC.GRID_STEPS_OUT and len(data) < len(plain)
    # before the merge: the pieces are joined, and the pen is lifted less often than there are squares
    Z = Dedup()
    merged, minfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(dedup=True, merge_paths=True), dedup_fn=Z, merge_fn=MD.merge_numpy, **GCODE_DOUBLES)
    assert minfo["merge"]["paths_in"] == info["dedup"]["paths_out"] == 9 and minfo["paths"] == minfo["merge"]["paths_out"] == len(MC.strokes_of(merged)) < 9
    assert down_steps(merged) == DC.GRID_STEPS_OUT
    lines = list(GC.report_lines("gcode", minfo))
    assert lines[0] == f"[gcode] dedup: 36 segments: 24 whole, 0 cut, 12 covered -> 9 strokes, pen-down steps {DC.GRID_STEPS_IN} -> {DC.GRID_STEPS_OUT}" and "merge:" in lines[1]
    # file order is kept with --no-reorder, and the pass is allowed there
    d3, i3 = GC.build_stream_from_gcode(text, GC.GcodeOptions(dedup=True, no_reorder=True), dedup_fn=Dedup(), **GCODE_DOUBLES)
    assert [s[0] for _, s in MC.strokes_of(d3)] == [tuple(out[1][a]) for a in out[0][:-1]]


def test_gcode_flow_with_pens_and_the_other_passes():
    """a stroke left in parts keeps its pen; strokes of different pens keep their ink; the simplification and the orders take what is left"""
    from orip import gcode as GC
    import clip_double as CD
    import merge_cases as MC
    import simplify_double as SD
    lines = ["G21 G90 M5"]
    paths = [(1, [(10, 10), (30, 10)]), (2, [(10, 10), (30, 10)]), (1, [(5, 10), (40, 10), (40, 20)]), (2, [(30, 10), (20, 10)]), (1, [(50, 50), (55, 50), (60, 50)])]
    for t, s in paths:
        lines += ["T%d" % t, "G0 X%g Y%g" % s[0], "M3"] + ["G1 X%g Y%g" % q for q in s[1:]] + ["M5"]
    text = "\n".join(lines) + "\n"
    Z = Dedup()
    dbl = dict(CD.gcode_doubles(), dedup_fn=Z, simplify_fn=SD.simplify_numpy)
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(dedup=True, tool_pens=True), **dbl)
    (off, pts, group, n_groups), out = Z.calls[0]
    assert n_groups == GC.MAX_PENS and group.tolist() == [1, 2, 1, 2, 1] and out[2].tolist() == [0, 1, 2, 2, 4]
    assert info["dedup"]["covered"] == 1 and info["dedup"]["cut"] == 1 and info["paths"] == 5
    by_pen = {}
    for c, s in MC.strokes_of(data):
        by_pen[c] = by_pen.get(c, 0) + sum(max(abs(q[0] - p[0]), abs(q[1] - p[1])) for p, q in zip(s[:-1], s[1:]))
    assert by_pen == {1: (35 + 10 + 10) * 40, 2: 20 * 40}
    d2, i2 = GC.build_stream_from_gcode(text, GC.GcodeOptions(dedup=True, tool_pens=True, merge_paths=True, allow_reverse=True, simplify_mm=0.0, improve_order=True), **dict(dbl, dedup_fn=Dedup()))
    assert i2["dedup"] == info["dedup"] and i2["merge"]["paths_in"] == 5 and i2["merge"]["joins"] == 2 and i2["simplify"]["points_out"] < i2["simplify"]["points_in"]
    assert down_steps(d2) == down_steps(data) == info["dedup"]["draw_steps_out"]


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def test_svg_flow_forwards_the_option():
    from orip import svg as SV
    plain, pinfo = SV.build_stream_from_svg(DC.tool_svg(), svg_options(DC.TOOL_SVG_ARGS[1:]), want_paths=True, **PD.pens_doubles())
    Z = Dedup()
    data, info = SV.build_stream_from_svg(DC.tool_svg(), svg_options(DC.TOOL_SVG_ARGS), want_paths=True, **dict(PD.pens_doubles(), dedup_fn=Z))
    d = info["dedup"]
    assert len(Z.calls) == 1 and Z.calls[0][0][3] == 8 and (d["segments"], d["whole"], d["covered"]) == (16, 14, 2)      # one border per pen; the one across the pens stays
    assert d["draw_steps_in"] - d["draw_steps_out"] == 2 * 20 * 40 == down_steps(plain) - down_steps(data)
    assert np.array_equal(info["fitted_paths"][1], pinfo["fitted_paths"][1])                   # the G-code file does not know of the pass
    d2, i2 = SV.build_stream_from_svg(DC.tool_svg(), svg_options(DC.TOOL_SVG_ARGS + ["--merge-paths", "--allow-reverse"]), **dict(PD.pens_doubles(), dedup_fn=Dedup(), merge_fn=MD.merge_numpy))
    assert i2["dedup"] == d and i2["merge"]["paths_in"] == d["paths_out"] == 4        # the merge takes what the dedup left


def test_a_return_that_does_not_hold_is_refused():
    from orip import gcode as GC
    text = DC.tool_gcode()
    good = DD.dedup_numpy

    def tampered(change):
        def fn(off, pts, group, n_groups):
            o, p, origin, st = good(off, pts, group, n_groups)
            return change(o.copy(), p.copy(), origin.copy(), dict(st))
        return fn
    def longer(o, p, g, s):
        """the last segment drawn 9000 steps further along its own axis, and the count of the pen-down steps out recounted: consistent, and more than went in"""
        q = p.copy(); q[-1] += 9000 * np.sign(q[-1] - q[-2])
        return o, q, g, dict(s, draw_steps_out=GC.draw_steps(o, q))
    wrong = {                                                                 # what is returned instead -> the check of _dedup that has to refuse it
        "origin descends": (lambda o, p, g, s: (o, p, g[::-1].copy(), s), "origins are not the input strokes"),
        "origin out of range": (lambda o, p, g, s: (o, p, np.r_[g[:-1], 9], s), "origins are not the input strokes"),
        "a stroke of one point": (lambda o, p, g, s: (np.r_[o[:1], o[1] - 1, o[1:]], p, np.r_[g[:1], g], dict(s, paths_out=s["paths_out"] + 1, pieces=s["pieces"] - 1)),
                                  "fewer than two points or with a repeated point"),
        "a repeated point": (lambda o, p, g, s: (o, np.r_[p[:1], p[:1], p[2:]], g, s), "fewer than two points or with a repeated point"),
        "counts": (lambda o, p, g, s: (o, p, g, dict(s, covered=s["covered"] + 1)), "counts do not add up"),
        "pieces": (lambda o, p, g, s: (o, p, g, dict(s, pieces=s["pieces"] + 1)), "counts do not add up"),
        "steps out": (lambda o, p, g, s: (o, p, g, dict(s, draw_steps_out=s["draw_steps_out"] - 1)), "counts do not add up"),
        "more ink": (longer, "the dedup added ink"),
    }
    GC.build_stream_from_gcode(text, GC.GcodeOptions(dedup=True), dedup_fn=tampered(lambda o, p, g, s: (o, p, g, s)), **GCODE_DOUBLES)
    for what, (change, message) in wrong.items():
        with pytest.raises(RuntimeError, match=message):
            GC.build_stream_from_gcode(text, GC.GcodeOptions(dedup=True), dedup_fn=tampered(change), **GCODE_DOUBLES)
            pytest.fail(what)


def test_the_tools_print_the_dedup_line(tmp_path, capsys):
    from orip import gcode as GC, svg as SV
    (tmp_path / "c.gcode").write_text(DC.tool_gcode())
    GC.main([str(tmp_path / "c.gcode"), "-o", str(tmp_path / "c.bin"), "--dedup"], **dict(GCODE_DOUBLES, dedup_fn=DD.dedup_numpy))
    assert f"[gcode] dedup: 36 segments: 24 whole, 0 cut, 12 covered -> 9 strokes, pen-down steps {DC.GRID_STEPS_IN} -> {DC.GRID_STEPS_OUT}" in capsys.readouterr().out
    (tmp_path / "d.svg").write_bytes(DC.tool_svg())
    SV.main_stream([str(tmp_path / "d.svg"), "--no-preview"] + DC.TOOL_SVG_ARGS, **dict(PD.pens_doubles(), dedup_fn=DD.dedup_numpy))
    assert "[svg] dedup: 16 segments: 14 whole, 0 cut, 2 covered -> " in capsys.readouterr().out and (tmp_path / "d_stream.bin").exists()
