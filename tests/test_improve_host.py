"""--improve-order on the host, without a GPU: invariants of the rule that need no second opinion, checked on the brute-force double
(tests/improve_double.py) round by round -- the sequence stays a permutation with its groups together, no stroke turns without reversal, the travel
falls by exactly the gain the round announced, and nothing is left to gain at the end; the moves the crafted plots must start with; and the host flow of
both tools with every device step injected as a double: the options parse and exclude what they must, the stream loses exactly the pen-up steps the
improvement reports, and without the option nothing is called and every byte is what it was.  No comparison here has a tolerance."""
import numpy as np
import pytest

import improve_cases as IC
import improve_double as ID
import gcode_double as D
import pens_double as PD
import svg_double as SD
import hatch_double as HD
from stream_double import codes_numpy

CASES = {"tiny_%d" % m: lambda r, m=m: IC.tiny(m, r) for m in range(5)}
CASES.update(identical=lambda r: IC.identical(), lattice=IC.lattice, corners=IC.corners, four_groups=IC.four_groups,
             random_65=lambda r: IC.random_plot(65, 3, reverse=r), random_3_groups=lambda r: IC.random_plot(80, 4, n_groups=3, reverse=r))


def never(*a, **k):
    raise AssertionError("the improvement was called without --improve-order")


def improve_double(ends, group, n_groups, order, rev, reverse, max_rounds):
    return ID.improve(ends, group, n_groups, order, rev, reverse, (0, 0), max_rounds)


def group_views(ends, group, n_groups, order, rev, start):
    """per non-empty group: (a, b, cursor) of the sequence as it stands"""
    a, b = ID.entries(ends, order, rev)
    og = np.asarray(group)[order]
    out, cursor = [], np.asarray(start, np.int64)
    for g in range(n_groups):
        pos = np.nonzero(og == g)[0]
        if len(pos):
            out.append((a[pos], b[pos], cursor))
            cursor = b[pos[-1]]
    return out


# ------------------------------------------------------------------ the rule, on the double
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_invariants_round_by_round(name, reverse):
    ends, group, ng, order, rev, start = CASES[name](reverse)
    n = len(order)
    whole_o, whole_r, whole = ID.improve(ends, group, ng, order, rev, reverse, start)
    rounds = 0
    for _ in range(2 * n + 70):
        announced = [ID.best_move(a, b, c, reverse)[0] for a, b, c in group_views(ends, group, ng, order, rev, start)]
        o2, r2, st = ID.improve(ends, group, ng, order, rev, reverse, start, 1)
        assert sorted(o2.tolist()) == list(range(n)) and (np.diff(group[o2]) >= 0).all() if n else True
        assert reverse or not r2.any()
        assert st["travel_before"] == ID.travel(ends, order, rev, start) and st["travel_after"] == ID.travel(ends, o2, r2, start)
        if st["rounds"] == 0:
            assert np.array_equal(o2, order) and np.array_equal(r2, rev) and all(g <= 0 for g in announced)
            break
        if ng == 1:                                                                # several groups: a later group's cursor moves with the group before it,
            assert st["rounds"] == 1 and announced[0] > 0                          # and the approach to it is in nobody's objective
            assert st["travel_after"] < st["travel_before"]                        # strictly, every round
            assert st["travel_before"] - st["travel_after"] == announced[0]        # the gain is the travel that goes
        order, rev, rounds = o2, r2, rounds + st["rounds"]
    else:
        raise AssertionError("the descent did not end")
    assert all(ID.best_move(a, b, c, reverse)[0] <= 0 for a, b, c in group_views(ends, group, ng, order, rev, start))
    if ng == 1:                                                                    # one call without a cap walks the same path
        assert np.array_equal(whole_o, order) and np.array_equal(whole_r, rev) and whole["rounds"] == rounds
    order, rev = whole_o, whole_r                                                  # group after group, each to its end: nothing left to gain either
    assert sorted(order.tolist()) == list(range(n)) and (n == 0 or (np.diff(group[order]) >= 0).all()) and (reverse or not rev.any())
    assert all(ID.best_move(a, b, c, reverse)[0] <= 0 for a, b, c in group_views(ends, group, ng, order, rev, start))
    assert whole["converged_groups"] == sum(1 for g in range(ng) if (group == g).any()) and whole["skipped_groups"] == 0
    assert whole["travel_after"] == ID.travel(ends, order, rev, start) <= whole["travel_before"]


@pytest.mark.parametrize("name", sorted(IC.FIRST_MOVES))
def test_crafted_first_moves(name):
    (ends, group, ng, order, rev, start), reverse, move = IC.FIRST_MOVES[name]
    trace = []
    ID.improve(ends, group, ng, order, rev, reverse, start, 1, trace=trace)
    assert len(trace) == 1 and trace[0][2:] == move and trace[0][1] > 0, trace


def test_caps_and_counts():
    ends, group, ng, order, rev, start = IC.random_plot(40, 9)
    assert ID.improve(ends, group, ng, order, rev, False, start, 0)[2]["converged_groups"] == 0          # nothing looked at, nothing converges
    o0, r0, s0 = ID.improve(ends, group, ng, order, rev, False, start, 0)
    assert np.array_equal(o0, order) and s0["travel_before"] == s0["travel_after"] and s0["rounds"] == 0
    full = ID.improve(ends, group, ng, order, rev, False, start)[2]
    assert 3 < full["rounds"] < 2 * 40 + 64 and full["converged_groups"] == 1
    capped = ID.improve(ends, group, ng, order, rev, False, start, full["rounds"])[2]                    # all the moves, but no round left to see the end
    assert capped["rounds"] == full["rounds"] and capped["converged_groups"] == 0 and capped["travel_after"] == full["travel_after"]
    assert ID.improve(ends, group, ng, order, rev, False, start, full["rounds"] + 1)[2] == full
    e, g, ng, o, r, st = IC.identical()
    o2, r2, s2 = ID.improve(e, g, ng, o, r, True, st)
    assert np.array_equal(o2, o) and not r2.any() and s2["rounds"] == 0 and s2["converged_groups"] == 1


def test_a_group_over_the_limit_is_left_alone(monkeypatch):
    monkeypatch.setattr(ID, "MAX_PATHS", 30)
    ends, group, ng, order, rev, start = IC.random_plot(50, 10, n_groups=2)
    group[:] = np.where(np.arange(50) < 35, 0, 1)
    order, rev = IC.sequence(group, np.random.default_rng(1))
    o2, r2, st = ID.improve(ends, group, 2, order, rev, False, start)
    assert st["skipped_groups"] == 1 and st["converged_groups"] == 1 and np.array_equal(o2[:35], order[:35]) and not np.array_equal(o2[35:], order[35:])


# ------------------------------------------------------------------ the command lines
def test_options_parse_on_both_tools():
    from orip import svg as SV, gcode as GC
    assert GC.GcodeOptions().improve_order is False and GC.GcodeOptions().improve_rounds is None
    assert SV.SvgOptions().improve_order is False and SV.SvgOptions().improve_rounds is None
    a = GC.build_argparser().parse_args(["in.gcode"])
    assert a.improve_order is False and a.improve_rounds is None
    o = GC.options_from_args(GC.build_argparser().parse_args(["in.gcode", "--improve-order", "--improve-rounds", "12"]))
    assert o.improve_order is True and o.improve_rounds == 12
    s = SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--improve-order", "--improve-rounds", "7", "--allow-reverse"]))
    assert s.improve_order is True and s.improve_rounds == 7
    g = SV.gcode_options(s)
    assert g.improve_order is True and g.improve_rounds == 7 and g.allow_reverse is True
    assert SV.gcode_options(SV.SvgOptions()).improve_order is False and SV.gcode_options(SV.SvgOptions()).improve_rounds is None
    ns = SV.build_gcode_argparser().parse_args(["in.svg"])
    assert not hasattr(ns, "improve_order") and not hasattr(ns, "improve_rounds")        # svg2gcode.py writes no stream


GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def test_option_errors():
    from orip import gcode as GC, svg as SV
    text = IC.tool_gcode(10)
    for o in (GC.GcodeOptions(improve_order=True, no_reorder=True), GC.GcodeOptions(improve_rounds=5), GC.GcodeOptions(improve_order=True, improve_rounds=-1)):
        with pytest.raises(ValueError):
            GC.build_stream_from_gcode(text, o, improve_fn=never, **GCODE_DOUBLES)
    for args in (["--improve-order", "--no-reorder"], ["--improve-rounds", "5"]):
        with pytest.raises(ValueError):
            SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(args), improve_fn=never, **PD.pens_doubles())
    with pytest.raises(ValueError):
        GC.main(["nowhere.gcode", "--improve-rounds", "3"])                       # before the file is looked for


# ------------------------------------------------------------------ the host flow through the doubles
class Improve:
    """the double, remembering what it was given"""
    def __init__(self): self.calls = []

    def __call__(self, ends, group, n_groups, order, rev, reverse, max_rounds):
        self.calls.append((np.array(ends), np.array(group), n_groups, np.array(order), np.array(rev), reverse, max_rounds))
        return improve_double(ends, group, n_groups, order, rev, reverse, max_rounds)


def gcode_modes():
    S = PD.StepsWithSource()
    pens = dict(GCODE_DOUBLES, steps_fn=S.steps, source_fn=S.source, order_pens_fn=PD.order_pens_numpy)
    return [("plain", {}, GCODE_DOUBLES), ("allow_reverse", {"allow_reverse": True}, pens)]


@pytest.mark.parametrize("mode", [0, 1])
def test_gcode_flow_saves_what_it_reports(mode):
    from orip import gcode as GC
    _, kw, dbl = gcode_modes()[mode]
    text = IC.tool_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(**kw), improve_fn=never, **dbl)
    I, tm = Improve(), {}
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(improve_order=True, **kw), improve_fn=I, timings=tm, **dbl)
    st = info["improve"]
    assert set(st) == set(ID.STAT_NAMES) and len(I.calls) == 1 and "improve" in tm and "improve" not in pinfo
    ends, group, ng, order, rev, reverse, cap = I.calls[0]
    assert ng == 1 and not group.any() and reverse is bool(kw.get("allow_reverse")) and cap is None and len(order) == info["paths"] == pinfo["paths"]
    assert reverse or not rev.any()
    assert st["travel_after"] < st["travel_before"] and st["converged_groups"] == 1 and st["skipped_groups"] == 0
    assert info["steps"] == pinfo["steps"] - (st["travel_before"] - st["travel_after"])      # the pen-up steps, and nothing else, went
    assert len(data) < len(plain)
    if mode:
        assert info["reversed"] == int(improve_double(*I.calls[0])[1].sum())                # the final directions
    capped, cinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(improve_order=True, improve_rounds=3, **kw), improve_fn=Improve(), **dbl)
    assert cinfo["improve"]["rounds"] == 3 and cinfo["improve"]["converged_groups"] == 0 and info["steps"] < cinfo["steps"] < pinfo["steps"]


def test_gcode_flow_with_tool_pens_and_merge():
    from orip import gcode as GC
    import merge_double as MD
    rng = np.random.default_rng(3)
    text = "\n".join(("T%d\n" % rng.integers(0, 3) + ln if ln.startswith("G0") else ln) for ln in IC.tool_gcode(60).split("\n"))
    S = PD.StepsWithSource()
    dbl = dict(GCODE_DOUBLES, steps_fn=S.steps, source_fn=S.source, order_pens_fn=PD.order_pens_numpy, merge_fn=MD.merge_numpy)
    base = dict(tool_pens=True, allow_reverse=True, merge_paths=True)
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(**base), improve_fn=never, **dbl)
    I = Improve()
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(improve_order=True, **base), improve_fn=I, **dbl)
    st = info["improve"]
    ends, group, ng, order, rev, reverse, cap = I.calls[0]
    assert ng == GC.MAX_PENS and reverse is True and sorted(set(group.tolist())) == [0, 1, 2] and (np.diff(group[order]) >= 0).all()
    assert len(order) == info["merge"]["paths_out"]                                        # the merged strokes are what is ordered
    assert st["converged_groups"] == 3 and st["travel_after"] < st["travel_before"]
    assert info["steps"] == pinfo["steps"] - (st["travel_before"] - st["travel_after"])
    assert info["pens"]["reversed"] == int(improve_double(*I.calls[0])[1].sum()) and info["pens"]["paths"] == pinfo["pens"]["paths"]


def test_svg_flow_saves_what_it_reports():
    from orip import svg as SV
    plain, pinfo = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS), improve_fn=never, **PD.pens_doubles())
    I = Improve()
    data, info = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS + ["--improve-order"]), improve_fn=I, **PD.pens_doubles())
    st = info["improve"]
    assert len(I.calls) == 1 and I.calls[0][2] == 8 and I.calls[0][5] is True
    assert st["travel_after"] < st["travel_before"] and st["converged_groups"] == 4
    assert info["steps"] == pinfo["steps"] - (st["travel_before"] - st["travel_after"]) and info["pens"]["paths"] == pinfo["pens"]["paths"]
    one, oinfo = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PLAIN_ARGS + ["--improve-order"]), improve_fn=Improve(), **dict(SD.svg_doubles(), hatch_fn=HD.hatch_numpy))
    p1, p1info = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PLAIN_ARGS), **dict(SD.svg_doubles(), hatch_fn=HD.hatch_numpy))
    assert oinfo["steps"] == p1info["steps"] - (oinfo["improve"]["travel_before"] - oinfo["improve"]["travel_after"]) < p1info["steps"]


def test_off_by_default_and_bytes_unchanged():
    from orip import gcode as GC, svg as SV
    from test_gcode_host import G, MAIN_CASES, options_for
    from test_pens_host import GP
    for i, (name, args) in enumerate(MAIN_CASES):
        data, info = GC.build_stream_from_gcode(bytes(G[f"text_{name}"]), options_for(args), improve_fn=never, **GCODE_DOUBLES)
        assert data == bytes(G[f"main_{i}_bin"]) and "improve" not in info
    data, info = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PLAIN_ARGS), improve_fn=never, **dict(SD.svg_doubles(), hatch_fn=HD.hatch_numpy))
    assert data == bytes(GP["tool_plain_stream"]) and "improve" not in info
    a = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS), **PD.pens_doubles())
    b = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS), improve_fn=never, **PD.pens_doubles())
    assert a[0] == b[0] and "improve" not in b[1]
