"""--loop-start on the host, without a GPU: the double of tests/seam_double.py against an exhaustive search over every assignment of seams, minimum and
lexicographic choice, on a few hundred tiny sequences; the consequences the rule lists, on the double; the rotation orip.gcode.gather_paths performs; and
the host flow of both tools with every device step injected as a double: the options parse, the pinned records stand, without the option nothing is
called and every byte is what the goldens hold, with it the stream loses exactly the pen-up steps the pass reports and nothing else moves.  No comparison
here has a tolerance."""
import numpy as np
import pytest

import seam_cases as SC
import seam_double as SD
import improve_double as ID
import gcode_double as D
import pens_double as PD
import svg_double as SVD
import hatch_double as HD
from stream_double import codes_numpy


def never(*a, **k):
    raise AssertionError("the seam pass was called without --loop-start")


# ------------------------------------------------------------------ the rule, on the double
@pytest.mark.parametrize("block", range(6))
def test_double_is_the_exhaustive_search(block):
    some_closed = some_tie = 0
    for seed in range(50 * block, 50 * block + 50):
        case = SC.tiny(seed)
        seam, st = SD.seams(*case)
        least, first = SD.exhaustive(*case)
        assert st["travel_after"] == least and seam.tolist() == first, seed
        assert st["travel_after"] == SD.travel(case[0], case[1], case[2], case[3], seam, case[4]) and st["travel_before"] == SD.travel(*case[:4], None, case[4])
        some_closed += st["closed"] > 0
        # how many assignments reach the minimum: where there are several, the lexicographic rule decided
        S = SD.strokes_of(case[0], case[1], case[2])
        alt = [list(seam) for _ in range(0)]
        for k, P in enumerate(S):
            if SD.is_closed(P):
                for v in range(len(P) - 1):
                    other = seam.copy(); other[k] = v
                    t = SD.travel(*case[:4], other, case[4])
                    assert t >= least                                            # one seam alone never lowers the travel
                    if v != seam[k] and t == least:
                        alt.append(other.tolist())
        some_tie += bool(alt)
        assert all(a > seam.tolist() for a in alt)
    assert some_closed > 25 and some_tie > 5


CASES = dict(SC.placements(), equidistant=SC.equidistant(), all_open=SC.all_open(), mixed_small=SC.mixed_small(), lattice=SC.lattice(), figure_eight=SC.figure_eight(),
             far_apart=SC.far_apart(), corners=SC.corners(), shuffled=SC.shuffled())


def segments(P):
    P = np.asarray(P, np.int64)
    return sorted(tuple(sorted((tuple(a), tuple(b)))) for a, b in zip(P[:-1].tolist(), P[1:].tolist()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_consequences_on_the_double(name):
    off, pts, order, rev, start = CASES[name]
    seam, st = SD.seams(off, pts, order, rev, start)
    S = SD.strokes_of(off, pts, order)
    n = len(S)
    closed = np.array([SD.is_closed(P) for P in S], bool)
    assert st["closed"] == int(closed.sum()) and st["moved"] == int((seam != 0).sum()) and not seam[~closed].any() and st["travel_after"] <= st["travel_before"]
    for k, P in enumerate(S):
        Q = SD.drawn(P, int(seam[k]), bool(rev[k]) if rev is not None else False)
        assert segments(Q) == segments(P) and len(Q) == len(P)
        if (np.abs(np.diff(P, axis=0)).max(1) > 0).all():
            assert (np.abs(np.diff(Q, axis=0)).max(1) > 0).all()                 # no stroke gains a repeated point
        if closed[k]:
            assert (Q[0] == P[seam[k]]).all() and (Q[-1] == P[seam[k]]).all()
    # idempotent: the pass on its own output finds nothing to move
    seq = np.arange(n) if order is None else np.asarray(order)
    from orip import gcode as GC
    goff, gpts = GC.gather_paths(off, pts, seq, rev, seam)
    again, st2 = SD.seams(goff, gpts, None, None, start)
    assert not again.any() and st2["travel_before"] == st2["travel_after"] == st["travel_after"]
    if not closed.any():
        assert st["travel_before"] == st["travel_after"] and np.array_equal(gpts, GC.gather_paths(off, pts, seq, rev)[1])


def test_named_answers():
    assert SD.seams(*SC.equidistant())[0].tolist() == [1]                         # vertices 1 and 2 tie: the lower one
    seam, st = SD.seams(*SC.figure_eight())
    assert seam[1] == 0 and st["closed"] == 3                                     # the cursor stands on vertices 0 and 4 of the eight: two candidates, the lower one
    assert SD.seams(*SC.far_apart())[1]["travel_after"] > 1 << 32
    runs = SC.placements()["two_runs"]                                            # runs do not depend on each other: each alone, from the cursor the open stroke leaves
    seam, _ = SD.seams(*runs)
    S = SD.strokes_of(runs[0], runs[1])
    tail = SC.pack([np.asarray(p) for p in S[3:]], start=tuple(S[2][-1].tolist()))
    assert SD.seams(*tail)[0].tolist() == seam[3:].tolist()
    head = SC.pack([np.asarray(p) for p in S[:3]])
    assert SD.seams(*head)[0].tolist() == seam[:3].tolist()


# ------------------------------------------------------------------ gather_paths
def test_gather_without_a_seam_is_the_old_call():
    from orip import gcode as GC
    off, pts, order, rev, _ = SC.shuffled()
    old = GC.gather_paths(off, pts, order, rev)
    for seam in (None, np.zeros(len(order), np.int32)):
        new = GC.gather_paths(off, pts, order, rev, seam)
        assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1]) and old[1].dtype == new[1].dtype
    new = GC.gather_paths(off, pts, order, seam=None)
    assert np.array_equal(new[1], GC.gather_paths(off, pts, order)[1])


@pytest.mark.parametrize("with_rev", [False, True])
def test_gather_rotates_as_the_rule_says(with_rev):
    from orip import gcode as GC
    off, pts, order, rev, start = SC.shuffled()
    rev = rev if with_rev else None
    seam, _ = SD.seams(off, pts, order, rev, start)
    assert (seam > 0).sum() > 10
    goff, gpts = GC.gather_paths(off, pts, order, rev, seam)
    S = SD.strokes_of(off, pts, order)
    assert np.array_equal(np.diff(goff), [len(P) for P in S])
    for k, P in enumerate(S):
        Q = gpts[goff[k]:goff[k + 1]]
        assert np.array_equal(Q, SD.drawn(P, int(seam[k]), bool(rev[k]) if with_rev else False))
        assert segments(Q) == segments(P) and (np.abs(np.diff(Q.astype(np.int64), axis=0)).max(1) > 0).all()
    assert GC.travel_steps(goff, gpts, start) == SD.travel(off, pts, order, rev, seam, start)


# ------------------------------------------------------------------ the command lines and the records
def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def test_options_parse_on_both_tools():
    from orip import svg as SV, gcode as GC
    assert GC.GcodeOptions().loop_start is False and SV.SvgOptions().loop_start is False
    assert GC.build_argparser().parse_args(["in.gcode"]).loop_start is False
    assert GC.options_from_args(GC.build_argparser().parse_args(["in.gcode", "--loop-start"])).loop_start is True
    assert GC.options_from_args(GC.build_argparser().parse_args(["in.gcode", "--loop-start", "--no-reorder"])).no_reorder is True
    GC.stroke_options(GC.GcodeOptions(loop_start=True, no_reorder=True))          # allowed: file order, better seams
    s = svg_options(["--loop-start", "--improve-order"])
    assert s.loop_start is True and SV.gcode_options(s).loop_start is True and SV.gcode_options(SV.SvgOptions()).loop_start is False
    assert svg_options([]).loop_start is False
    assert not hasattr(SV.build_gcode_argparser().parse_args(["in.svg"]), "loop_start")      # svg2gcode.py writes no stream
    with pytest.raises(SystemExit):
        SV.build_gcode_argparser().parse_args(["in.svg", "--loop-start"])


def test_pinned_records_stand():
    from orip import svg as SV, gcode as GC
    import recording_device as RD
    gcode_steps, svg_steps = RD.doors_take_the_pass_table()
    assert "seam_fn" in gcode_steps and "seam_fn" in svg_steps and GC.PASSES[-1].name == "seam"
    assert len(GC.STROKE_ARGS) == 10 and GC.STROKE_ARGS[-1] == "--dedup" and "--loop-start" not in GC.STROKE_ARGS
    g = list(GC.GcodeOptions.__dataclass_fields__)
    assert g[-2:] == ["dash_mm", "dash_offset_mm"] and g[-3] == "loop_start"
    s = list(SV.SvgOptions.__dataclass_fields__)
    assert s[-1] == "dashes" and "loop_start" in s[:-1]
    assert GC.SEAM_STATS == SD.STAT_NAMES
    from orip import lib
    assert lib.SEAM_STATS == SD.STAT_NAMES and "orip_gcode_seam" in lib.SIGNATURES
    assert "seam" not in list(GC.report_lines("x", {"improve": dict.fromkeys(GC.IMPROVE_STATS, 0)}))[-1]
    st = dict(closed=3, moved=2, travel_before=50, travel_after=41)
    assert list(GC.report_lines("x", {"seam": st}))[-1] == GC.seam_line("x", st) and "50 -> 41 (9 saved)" in GC.seam_line("x", st)


# ------------------------------------------------------------------ the host flow through the doubles
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)


class Seam:
    """the double, remembering what it was given"""
    def __init__(self): self.calls = []

    def __call__(self, off, pts, order, rev):
        self.calls.append((np.array(off), np.array(pts), None if order is None else np.array(order), None if rev is None else np.array(rev)))
        return SD.seams(off, pts, order, rev, (0, 0))


def improve_double(ends, group, n_groups, order, rev, reverse, max_rounds):
    return ID.improve(ends, group, n_groups, order, rev, reverse, (0, 0), max_rounds)


@pytest.mark.parametrize("mode", ["plain", "no_reorder", "improve", "allow_reverse"])
def test_gcode_flow_saves_what_it_reports(mode):
    from orip import gcode as GC
    S = PD.StepsWithSource()
    kw, dbl = {}, dict(GCODE_DOUBLES, improve_fn=improve_double)
    if mode == "no_reorder": kw = dict(no_reorder=True)
    if mode == "improve": kw = dict(improve_order=True)
    if mode == "allow_reverse": kw, dbl = dict(allow_reverse=True, improve_order=True), dict(dbl, steps_fn=S.steps, source_fn=S.source, order_pens_fn=PD.order_pens_numpy)
    text = SC.tool_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(**kw), seam_fn=never, **dbl)
    F, tm = Seam(), {}
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(loop_start=True, **kw), seam_fn=F, timings=tm, **dbl)
    st = info["seam"]
    assert set(st) == set(SD.STAT_NAMES) and len(F.calls) == 1 and "seam" in tm and "seam" not in pinfo
    off, pts, order, rev = F.calls[0]
    assert len(off) - 1 == info["paths"] == pinfo["paths"] == 30 and st["closed"] == 20 and st["moved"] >= 1
    assert (order is None) == (mode == "no_reorder") and (rev is None or mode == "allow_reverse" or not rev.any())
    assert st["travel_after"] < st["travel_before"]
    assert info["steps"] == pinfo["steps"] - (st["travel_before"] - st["travel_after"])      # the pen-up steps, and nothing else, went
    assert info["moves"] == pinfo["moves"] and {k: info[k] for k in ("paths_mm", "pen_down_moves", "target")} == {k: pinfo[k] for k in ("paths_mm", "pen_down_moves", "target")}
    if "improve" in info:
        assert info["improve"] == pinfo["improve"] and st["travel_before"] == info["improve"]["travel_after"]
    if mode == "allow_reverse":
        assert info["reversed"] == pinfo["reversed"]
    assert list(GC.report_lines("gcode", info))[-1] == GC.seam_line("gcode", st)


def test_a_seam_that_breaks_the_rule_is_refused():
    from orip import gcode as GC
    text = SC.tool_gcode()

    def wrong(how):
        def fn(off, pts, order, rev):
            seam, st = SD.seams(off, pts, order, rev, (0, 0))
            seam = seam.copy(); st = dict(st)
            if how == "open": seam[int(np.nonzero(np.diff(off)[order] == 14)[0][0])] = 1       # the circle with a tail is open
            if how == "range": seam[int(np.nonzero(np.diff(off)[order] == 5)[0][0])] = 4
            if how == "count": st["moved"] += 1
            if how == "travel": st["travel_after"] -= 1
            if how == "short": seam = seam[:-1]
            return seam, st
        return fn
    for how in ("open", "range", "count", "travel", "short"):
        with pytest.raises(RuntimeError):
            GC.build_stream_from_gcode(text, GC.GcodeOptions(loop_start=True), seam_fn=wrong(how), **GCODE_DOUBLES)


def test_svg_flow_saves_what_it_reports():
    from orip import svg as SV
    for args, dbl in ((SC.TOOL_SVG_ARGS + ["--improve-order"], lambda: dict(PD.pens_doubles(), improve_fn=improve_double)), ([], SVD.svg_doubles), (["--no-reorder"], SVD.svg_doubles)):
        plain, pinfo = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(args), seam_fn=never, want_paths=True, **dbl())
        F = Seam()
        data, info = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(args + ["--loop-start"]), seam_fn=F, want_paths=True, **dbl())
        st = info["seam"]
        assert len(F.calls) == 1 and st["closed"] == 12 and st["moved"] >= 1 and st["travel_after"] < st["travel_before"]      # circles, rectangles and closed paths
        assert info["steps"] == pinfo["steps"] - (st["travel_before"] - st["travel_after"]) and info["paths"] == pinfo["paths"] == 16
        assert info.get("pens") == pinfo.get("pens") and info.get("improve") == pinfo.get("improve")
        assert all(np.array_equal(a, b) for a, b in zip(info["fitted_paths"], pinfo["fitted_paths"]))       # the G-code file is what it was
        assert list(SV.GC.report_lines("svg", info))[-1] == SV.GC.seam_line("svg", st)
    data, info = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS + ["--loop-start"]), seam_fn=Seam(), **PD.pens_doubles())
    assert info["seam"]["closed"] == 2                                              # the circle and the rectangle of the older drawing; its hatch lines are open


def test_off_by_default_and_bytes_unchanged():
    from orip import gcode as GC, svg as SV
    from test_gcode_host import G, MAIN_CASES, options_for
    from test_svg_host import G as GS, ARGS, RUNS, options_for as svg_options_for
    from test_pens_host import GP
    for i, (name, args) in enumerate(MAIN_CASES):
        data, info = GC.build_stream_from_gcode(bytes(G[f"text_{name}"]), options_for(args), seam_fn=never, **GCODE_DOUBLES)
        assert data == bytes(G[f"main_{i}_bin"]) and "seam" not in info
    for i, (name, key) in enumerate(RUNS):
        data, info = SV.build_stream_from_svg(bytes(GS[f"svg_{name}"]), svg_options_for(ARGS[key]), seam_fn=never, **SVD.svg_doubles())
        assert data == bytes(GS[f"run_{i}_bin"]) and "seam" not in info
    data, info = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PLAIN_ARGS), seam_fn=never, **dict(SVD.svg_doubles(), hatch_fn=HD.hatch_numpy))
    assert data == bytes(GP["tool_plain_stream"]) and "seam" not in info
    a = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS), **PD.pens_doubles())
    b = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS), seam_fn=never, **PD.pens_doubles())
    assert a[0] == b[0] and "seam" not in b[1]
