"""--merge-paths on the host, without a GPU: invariants of the rule that need no second opinion, checked on the sequential double (tests/merge_double.py) for
the crafted shapes and a random drawing, each with and without REVERSE; and the host flow of both tools with every device step injected as a double: the
option parses, without it nothing is called and every byte is what it was, with it the pens stay apart, the order rules hold and info["merge"] is right.
No comparison here has a tolerance."""
from collections import Counter

import numpy as np
import pytest

import merge_cases as MC
import merge_double as MD
import gcode_double as D
import pens_double as PD
import svg_double as SD
from stream_double import codes_numpy

CASES = dict(MC.small_cases(), random_grid=MC.random_grid())


def never(*a, **k):
    raise AssertionError("the merge was called without --merge-paths")


def segments(off, pts):
    """the multiset of undirected segments (consecutive point pairs) of a set of paths"""
    pts = np.asarray(pts, np.int64)
    inner = np.ones(len(pts), bool); inner[np.asarray(off[1:], np.int64) - 1] = False
    a, b = pts[:-1][inner[:-1]], pts[1:][inner[:-1]]
    swap = (a[:, 0] > b[:, 0]) | ((a[:, 0] == b[:, 0]) & (a[:, 1] > b[:, 1]))
    lo, hi = np.where(swap[:, None], b, a), np.where(swap[:, None], a, b)
    return Counter(map(tuple, np.concatenate([lo, hi], 1).tolist()))


# ------------------------------------------------------------------ the rule, on the double
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_invariants(name, reverse):
    off, pts, group, ng = CASES[name]
    n = len(off) - 1
    o2, p2, moff, member, rev, st = MD.merge_numpy(off, pts, group, ng, reverse)
    m = len(o2) - 1
    assert st == {"paths_out": m, "points_out": len(p2), "joins": n - m, "cycles": st["cycles"]} and int(o2[-1]) == len(p2)
    assert len(moff) == m + 1 and moff[0] == 0 and moff[-1] == n and sorted(member.tolist()) == list(range(n)) and len(rev) == n
    assert segments(o2, p2) == segments(off, pts)                                          # nothing drawn twice, nothing lost
    same = (np.diff(p2, axis=0) == 0).all(1); same[o2[1:-1] - 1] = False
    assert not same.any()                                                                  # no two equal consecutive points inside a path
    degree = Counter()
    for p in range(n):
        degree[(int(group[p]), *pts[off[p]].tolist())] += 1; degree[(int(group[p]), *pts[off[p + 1] - 1].tolist())] += 1
    lens = np.diff(off)
    for c in range(m):
        mem = member[moff[c]:moff[c + 1]]
        assert len(set(group[mem].tolist())) == 1                                          # one pen per output path
        at = int(o2[c])
        for k, p in enumerate(mem.tolist()):
            seg = pts[off[p]:off[p + 1]][::-1] if rev[moff[c] + k] else pts[off[p]:off[p + 1]]
            at += 0 if k == 0 else -1
            assert np.array_equal(p2[at:at + lens[p]], seg)                                # every member in place, whole, in the direction rev states
            if k:
                assert degree[(int(group[p]), *p2[at].tolist())] == 2                      # an interior joint: exactly two ends met there, in one group
            at += int(lens[p])
        assert at == o2[c + 1]
    if not reverse:
        assert not rev.any()
    lowest = [int(member[moff[c]:moff[c + 1]].min()) for c in range(m)]
    assert lowest == sorted(lowest) and len(set(lowest)) == m                              # output paths ascend by lowest member
    again = MD.merge_numpy(o2, p2, group[member[moff[:-1]]], ng, reverse)                   # a second merge joins nothing
    assert again[5]["joins"] == 0 and np.array_equal(again[0], o2) and np.array_equal(again[1], p2)


def test_expected_joins_of_the_small_shapes():
    want = {"one_open": (0, 0), "one_closed": (0, 0), "tail_head": (1, 1), "tail_tail": (0, 1), "head_head": (0, 1), "three_on_a_node": (1, 2), "closed_plus_end": (0, 0),
            "two_cycle": (1, 1), "two_cycle_reverse_only": (0, 1), "three_cycle": (2, 2), "duplicate": (0, 1), "two_groups": (0, 0), "x_only": (0, 0), "y_only": (0, 0),
            "swapped": (0, 0), "group_only": (1, 1), "corners": (2, 2), "cycle_64_forwards": (63, 63), "chain_65": (None, 64), "cycle_257": (None, 256)}
    for name, (plain, rev) in want.items():
        off, pts, group, ng = CASES[name]
        for reverse, joins in ((False, plain), (True, rev)):
            if joins is not None:
                assert MD.merge_numpy(off, pts, group, ng, reverse)[5]["joins"] == joins, (name, reverse)
    for name, cyc in (("two_cycle", (1, 1)), ("three_cycle", (1, 1)), ("duplicate", (0, 1)), ("two_cycle_reverse_only", (0, 1)), ("cycle_1025", (0, 1)), ("cycle_1025_forwards", (1, 1)),
                      ("corners", (0, 0))):
        off, pts, group, ng = CASES[name]
        assert tuple(MD.merge_numpy(off, pts, group, ng, r)[5]["cycles"] for r in (False, True)) == cyc, name


def test_cycle_starts_at_its_lowest_member_forwards():
    off, pts, group, ng = CASES["three_cycle"]                                              # file: lone, ring 1, ring 2, ring 0, lone
    o2, p2, moff, member, rev, st = MD.merge_numpy(off, pts, group, ng, True)
    assert member.tolist() == [0, 1, 2, 3, 4] and not rev.any() and moff.tolist() == [0, 1, 4, 5]
    ring = p2[o2[1]:o2[2]]
    assert np.array_equal(ring[0], ring[-1]) and np.array_equal(ring[:2], pts[off[1]:off[2]]) and len(ring) == 4
    off, pts, group, ng = CASES["duplicate"]
    _, p2, _, member, rev, _ = MD.merge_numpy(off, pts, group, ng, True)
    assert member.tolist() == [0, 1] and rev.tolist() == [False, True] and p2.tolist() == [[5, 5], [9, 1], [9, 9], [9, 1], [5, 5]]


def test_unchanged_without_coincident_ends():
    rng = np.random.default_rng(2)
    lens = rng.integers(2, 6, 300)
    off = np.concatenate([[0], np.cumsum(lens)])
    pts = np.stack([np.arange(off[-1]) * 2, rng.integers(0, 1000, off[-1])], 1).astype(np.int32)     # every x once: no two points coincide
    for reverse in (False, True):
        o2, p2, moff, member, rev, st = MD.merge_numpy(off, pts, rng.integers(0, 3, 300), 3, reverse)
        assert np.array_equal(o2, off) and np.array_equal(p2, pts) and np.array_equal(moff, np.arange(301)) and np.array_equal(member, np.arange(300))
        assert not rev.any() and st == {"paths_out": 300, "points_out": int(off[-1]), "joins": 0, "cycles": 0}
    o2, p2, moff, member, rev, st = MD.merge_numpy([0], np.zeros((0, 2)), [], 1)
    assert o2.tolist() == [0] and p2.shape == (0, 2) and moff.tolist() == [0] and len(member) == 0 and st["paths_out"] == 0


# ------------------------------------------------------------------ the command lines
def test_option_parses_on_both_tools():
    from orip import svg as SV, gcode as GC
    assert GC.GcodeOptions().merge_paths is False and SV.SvgOptions().merge_paths is False
    assert GC.build_argparser().parse_args(["in.gcode"]).merge_paths is False and SV.build_stream_argparser().parse_args(["in.svg"]).merge_paths is False
    assert GC.options_from_args(GC.build_argparser().parse_args(["in.gcode", "--merge-paths"])).merge_paths is True
    o = SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--merge-paths", "--allow-reverse"]))
    assert o.merge_paths is True and SV.gcode_options(o).merge_paths is True and SV.gcode_options(o).allow_reverse is True
    assert SV.gcode_options(SV.SvgOptions()).merge_paths is False
    assert not hasattr(SV.build_gcode_argparser().parse_args(["in.svg"]), "merge_paths")      # svg2gcode.py writes G-code: the merge lives in the stream


# ------------------------------------------------------------------ the host flow through the doubles
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)


class Merge:
    """merge_double.merge_numpy that remembers what it was given and what it returned"""
    def __init__(self): self.calls = []

    def __call__(self, off, pts, group, n_groups, reverse):
        out = MD.merge_numpy(off, pts, group, n_groups, reverse)
        self.calls.append(((np.array(off), np.array(pts), np.array(group), n_groups, reverse), out))
        return out


def test_off_by_default_and_bytes_unchanged():
    from orip import gcode as GC, svg as SV
    from test_gcode_host import G, MAIN_CASES, options_for
    for i, (name, args) in enumerate(MAIN_CASES):
        data, info = GC.build_stream_from_gcode(bytes(G[f"text_{name}"]), options_for(args), merge_fn=never, **GCODE_DOUBLES)
        assert data == bytes(G[f"main_{i}_bin"]) and "merge" not in info
    text = MC.tool_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(), **GCODE_DOUBLES)
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(merge_paths=False), merge_fn=never, **GCODE_DOUBLES)
    assert data == plain and info == pinfo
    o = SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview", "--pen-colors", "#f00,#00f"]))
    a = SV.build_stream_from_svg(MC.tool_svg(), o, **PD.pens_doubles())
    b = SV.build_stream_from_svg(MC.tool_svg(), o, merge_fn=never, **PD.pens_doubles())
    assert a[0] == b[0] and "merge" not in b[1]


def test_gcode_flow_merges_before_the_order():
    from orip import gcode as GC
    text = MC.tool_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(), **GCODE_DOUBLES)
    M = Merge()
    tm = {}
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(merge_paths=True), merge_fn=M, timings=tm, **GCODE_DOUBLES)
    (off, pts, group, ng, reverse), out = M.calls[0]
    assert len(M.calls) == 1 and ng == 1 and reverse is False and not group.any() and len(group) == pinfo["paths"] == 8 + 299 and "merge" in tm
    # the square: two strokes of two sides each (three ends meet on the diagonal's corners); the diagonal; the triangle, closed; the sine, whole
    assert info["merge"] == {"paths_in": 307, "paths_out": 5, "joins": 302, "cycles": 1} and out[5]["joins"] == 302
    assert info["paths"] == 5
    got, was = MC.strokes_of(data), MC.strokes_of(plain)
    assert len(was) == 307 and len(got) == 5 == len(was) - info["merge"]["joins"]
    assert sum(len(s) - 1 for _, s in got) == sum(len(s) - 1 for _, s in was)                # the pen draws the same steps
    assert sorted(np.diff(out[2]).tolist()) == [1, 2, 2, 3, 299]                            # the diagonal, the square's halves, the triangle, the sine in one stroke
    closed = [s for _, s in got if s[0] == s[-1]]
    assert len(closed) == 1 and len(set(closed[0])) > 50                                    # the triangle comes back closed
    # --no-reorder: the merged paths in the order of their lowest members
    d2, i2 = GC.build_stream_from_gcode(text, GC.GcodeOptions(merge_paths=True, no_reorder=True), merge_fn=Merge(), order_fn=never, **{k: v for k, v in GCODE_DOUBLES.items() if k != "order_fn"})
    o2, p2 = out[0], out[1]
    assert [s[0] for _, s in MC.strokes_of(d2)] == [tuple(p2[a].tolist()) for a in o2[:-1]] and i2["merge"] == info["merge"]


def test_allow_reverse_reaches_the_merge():
    from orip import gcode as GC
    lines = ["G21 G90 M5"]
    for a, b in (((10, 10), (20, 10)), ((30, 10), (20, 10)), ((30, 10), (30, 30))):             # the middle stroke runs the other way
        lines += ["G0 X%g Y%g" % a, "M3", "G1 X%g Y%g" % b, "M5"]
    text = "\n".join(lines) + "\n"
    S = PD.StepsWithSource()
    dbl = dict(GCODE_DOUBLES, steps_fn=S.steps, source_fn=S.source, order_pens_fn=PD.order_pens_numpy)
    M = Merge()
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(merge_paths=True, allow_reverse=True), merge_fn=M, **dbl)
    assert M.calls[0][0][3:] == (1, True) and info["merge"] == {"paths_in": 3, "paths_out": 1, "joins": 2, "cycles": 0} and len(MC.strokes_of(data)) == 1
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(merge_paths=True), merge_fn=Merge(), **GCODE_DOUBLES)
    assert info["merge"]["joins"] == 0 and len(MC.strokes_of(data)) == 3


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def test_svg_flow_keeps_the_pens_apart():
    from orip import svg as SV
    M = Merge()
    data, info = SV.build_stream_from_svg(MC.tool_svg(), svg_options(MC.TOOL_SVG_ARGS), merge_fn=M, **PD.pens_doubles())
    (off, pts, group, ng, reverse), out = M.calls[0]
    assert ng == 8 and reverse is False and sorted(set(group.tolist())) == [0, 1] and (group[:8] == 0).all() and (group[8:] == 1).all()
    assert info["merge"] == {"paths_in": 307, "paths_out": 5, "joins": 302, "cycles": 1}
    moff, member = out[2], out[3]
    assert all(len(set(group[member[a:b]].tolist())) == 1 for a, b in zip(moff[:-1], moff[1:]))
    got = MC.strokes_of(data)
    assert [c for c, _ in got] == [0, 0, 0, 0, 1]                                           # four red strokes, then the sine in blue: the members' pens
    assert info["pens"]["paths"][:2] == [8, 299]                                            # counted per input path, as before
    # a blue line laid on a red joint does not take part: the groups differ
    extra = MC.tool_svg().replace(b"</svg>", b'<line x1="60" y1="10" x2="90" y2="5" stroke="#00f"/></svg>')
    d2, i2 = SV.build_stream_from_svg(extra, svg_options(MC.TOOL_SVG_ARGS), merge_fn=Merge(), **PD.pens_doubles())
    assert i2["merge"] == {"paths_in": 308, "paths_out": 6, "joins": 302, "cycles": 1}
    # --no-reorder with pens: pen after pen, inside a pen the order of the lowest members
    M3 = Merge()
    d3, i3 = SV.build_stream_from_svg(MC.tool_svg(), svg_options(MC.TOOL_SVG_ARGS + ["--no-reorder"]), merge_fn=M3, **dict(PD.pens_doubles(), order_pens_fn=never))
    o3, p3 = M3.calls[0][1][0], M3.calls[0][1][1]
    assert [s[0] for _, s in MC.strokes_of(d3)] == [tuple(p3[a].tolist()) for a in o3[:-1]]


def test_hatch_lines_go_through_the_merge():
    """without serpentine every hatch line of a rectangle is a stroke of its own and none touch: the merge sees them and joins none"""
    from orip import svg as SV
    import hatch_double as HD
    src = b'<svg xmlns="http://www.w3.org/2000/svg" width="100" height="100"><rect x="10" y="10" width="60" height="40" fill="#000" stroke="#000"/></svg>'
    M = Merge()
    data, info = SV.build_stream_from_svg(src, svg_options(["--merge-paths", "--hatch-spacing-mm", "2.0"]), merge_fn=M, **dict(SD.svg_doubles(), hatch_fn=HD.hatch_numpy))
    assert info["hatch"]["segments"] > 5 and info["merge"]["paths_in"] == 1 + info["hatch"]["segments"] and info["merge"]["joins"] == 0
