"""--ring-entry on the host, without a GPU: the double of tests/ring_entry_double.py against the doubles of the plain orders where no stroke is closed and
against answers worked out by hand; then the host flow of both tools with every device step injected as a double: the option parses, the call stands in
the greedy order's place, the rings are rotated before --improve-order and --loop-start see them, the travel the call reports is the travel of the strokes as
gathered, a result that breaks the rule is refused, and without the option nothing is called and every byte is what it was.  No comparison has a tolerance."""
import numpy as np
import pytest

import seam_cases as SC
import seam_double as SD
import ring_entry_double as RD
import improve_double as ID
import gcode_double as D
import pens_double as PD
import svg_double as SVD
from stream_double import codes_numpy


def never(*a, **k):
    raise AssertionError("the ring order was called without --ring-entry")


def ends_of(off, pts):
    return np.concatenate([pts[off[:-1]], pts[off[1:] - 1]], 1)


# ------------------------------------------------------------------ the double itself
@pytest.mark.parametrize("seed", range(6))
def test_double_is_the_plain_order_without_rings(seed):
    rng = np.random.default_rng(seed)
    n = 60
    strokes = [rng.integers(0, 40, (int(rng.integers(1, 5)), 2)) for _ in range(n)]              # a coarse lattice: ties everywhere; 1-point strokes and A, B, A
    strokes += [np.array([a, b, a]) for a, b in rng.integers(0, 40, (5, 2, 2))]
    off, pts, _, _, _ = SC.pack(strokes)
    ends = ends_of(off, pts)
    grp = rng.integers(0, 3, len(strokes)).astype(np.int32)
    start = tuple(int(v) for v in rng.integers(0, 40, 2))
    for reverse in (False, True):
        order, rev, seam, st = RD.order_rings(off, pts, grp, 3, reverse, start)
        want = PD.order_pens_numpy(ends, grp, 3, reverse, start)
        assert np.array_equal(order, want[0]) and np.array_equal(rev, want[1]) and not seam.any()
        assert st == dict(closed=0, moved=0, candidates=len(strokes) * (1 + reverse), travel=SD.travel(off, pts, order, rev, None, start))
    order, rev, seam, _ = RD.order_rings(off, pts)
    assert np.array_equal(order, D.order_numpy(ends)) and not rev.any()


def test_hand_worked_answers():
    a = np.array([[20, 20], [10, 20], [10, 10], [20, 10], [20, 20]])                         # stored from its far corner: (10, 10) is vertex 2
    b = np.array([[50, 20], [40, 20], [40, 10], [50, 10], [50, 20]])                         # from (10, 10) the nearest is (40, 10), vertex 2
    off, pts, _, _, _ = SC.pack([a, b])
    order, rev, seam, st = RD.order_rings(off, pts)
    assert (order.tolist(), rev.tolist(), seam.tolist()) == ([0, 1], [False, False], [2, 2]) and st == dict(closed=2, moved=2, candidates=8, travel=10 + 30)
    assert RD.order_rings(off, pts, reverse=True)[3]["candidates"] == 8                      # a closed stroke has no reverse candidate
    # the plain order walks to the stored first vertices: (20, 20), then (50, 20)
    assert SD.travel(off, pts, D.order_numpy(ends_of(off, pts))) == 20 + 30
    off, pts, _, _, start = SC.equidistant()                                                 # vertices 1 and 2 are both 30 away in L1: the lower one
    order, rev, seam, st = RD.order_rings(off, pts, start=start)
    assert seam.tolist() == [1] and st["travel"] == 20 and st["moved"] == 1
    off, pts, _, _, _ = SC.pack([SC.square(30, 30, 10), SC.square(5, 5, 10), SC.square(30, 30, 10)])      # two coincident rings: the lower stroke first
    order, rev, seam, st = RD.order_rings(off, pts)
    assert order.tolist() == [1, 0, 2] and seam.tolist() == [0, 0, 0] and st["travel"] == 5 + 25 + 0      # from (5, 5) the nearest is (30, 30), 50 away
    off, pts, _, _, _ = SC.figure_eight()                                                    # the cursor stands on vertices 0 and 4 of the eight: the lower one
    order, rev, seam, st = RD.order_rings(off, pts)
    assert order.tolist() == [0, 1, 2, 3] and seam.tolist() == [0, 0, 0, 1] and st["closed"] == 3 and st["candidates"] == 1 + 8 + 4 + 8
    # (110, 110) and (100, 120) of the far eight are both 140 from (60, 20): vertex 1 before vertex 2


def test_double_on_mixed_inputs_keeps_the_rule():
    for case in (SC.mixed_small(), SC.lattice(), SC.shuffled(), SC.corners(), SC.far_apart()):
        off, pts, _, _, start = case
        n = len(off) - 1
        grp = (np.arange(n) % 3).astype(np.int32)
        for reverse in (False, True):
            order, rev, seam, st = RD.order_rings(off, pts, grp, 3, reverse, start)
            S = SD.strokes_of(off, pts, order)
            closed = np.array([SD.is_closed(P) for P in S], bool)
            assert sorted(order.tolist()) == list(range(n)) and (np.diff(grp[order]) >= 0).all() and not rev[closed].any() and not seam[~closed].any()
            assert all(0 <= int(seam[k]) < len(S[k]) - 1 for k in np.nonzero(closed)[0])
            assert st["travel"] == SD.travel(off, pts, order, rev, seam, start) and st["closed"] == int(closed.sum())


# ------------------------------------------------------------------ the command lines and the records
def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def test_options_parse_and_no_reorder_is_an_argument_error():
    from orip import svg as SV, gcode as GC
    assert GC.GcodeOptions().ring_entry is False and SV.SvgOptions().ring_entry is False
    assert GC.options_from_args(GC.build_argparser().parse_args(["in.gcode"])).ring_entry is False
    assert GC.options_from_args(GC.build_argparser().parse_args(["in.gcode", "--ring-entry"])).ring_entry is True
    s = svg_options(["--ring-entry", "--loop-start"])
    assert s.ring_entry is True and SV.gcode_options(s).ring_entry is True and SV.gcode_options(SV.SvgOptions()).ring_entry is False
    assert not hasattr(SV.build_gcode_argparser().parse_args(["in.svg"]), "ring_entry")      # svg2gcode.py writes no stream
    with pytest.raises(SystemExit):
        SV.build_gcode_argparser().parse_args(["in.svg", "--ring-entry"])
    with pytest.raises(ValueError, match="--ring-entry with --no-reorder"):
        GC.stroke_options(GC.GcodeOptions(ring_entry=True, no_reorder=True))
    with pytest.raises(ValueError, match="--ring-entry with --no-reorder"):
        GC.build_stream_from_gcode(SC.tool_gcode(), GC.GcodeOptions(ring_entry=True, no_reorder=True), ring_entry_fn=never, **GCODE_DOUBLES)
    with pytest.raises(ValueError, match="--ring-entry with --no-reorder"):
        SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(["--ring-entry", "--no-reorder"]), ring_entry_fn=never, **SVD.svg_doubles())
    from orip import lib
    assert GC.RING_ENTRY_STATS == lib.RING_ENTRY_STATS == RD.STAT_NAMES and "orip_gcode_order_rings" in lib.SIGNATURES
    import recording_device as REC
    gcode_steps, svg_steps = REC.doors_take_the_pass_table()
    assert "ring_entry_fn" in gcode_steps and "ring_entry_fn" in svg_steps and "--ring-entry" not in GC.STROKE_ARGS


# ------------------------------------------------------------------ the host flow through the doubles
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)


class Rings:
    """the double, remembering what it was given and what it answered"""
    def __init__(self): self.calls = []

    def __call__(self, off, pts, group, n_groups, reverse):
        out = RD.order_rings(off, pts, group, n_groups, reverse)
        self.calls.append((np.array(off), np.array(pts), np.array(group), n_groups, reverse, out))
        return out

    def entered(self):
        """the strokes as the flow must hand them on: every ring rotated in place to the vertex it was entered at"""
        off, pts, _, _, _, (order, rev, seam, _) = self.calls[0]
        out = pts.copy()
        for k, i in enumerate(order.tolist()):
            out[off[i]:off[i + 1]] = SD.drawn(pts[off[i]:off[i + 1]], int(seam[k]), False)
        return out


class Seam:
    def __init__(self): self.calls = []

    def __call__(self, off, pts, order, rev):
        self.calls.append((np.array(off), np.array(pts), None if order is None else np.array(order), None if rev is None else np.array(rev)))
        return SD.seams(off, pts, order, rev, (0, 0))


class Improve:
    def __init__(self): self.calls = []

    def __call__(self, ends, group, n_groups, order, rev, reverse, max_rounds):
        self.calls.append((np.array(ends), np.array(order), np.array(rev)))
        return ID.improve(ends, group, n_groups, order, rev, reverse, (0, 0), max_rounds)


@pytest.mark.parametrize("mode", ["alone", "loop_start", "improve", "all"])
def test_gcode_flow_rotates_before_improve_and_seam(mode):
    from orip import gcode as GC
    S = PD.StepsWithSource()
    kw, dbl = {}, dict(GCODE_DOUBLES)
    if mode in ("loop_start", "all"): kw["loop_start"] = True
    if mode in ("improve", "all"): kw["improve_order"] = True
    if mode == "all": kw["allow_reverse"] = True; dbl.update(steps_fn=S.steps, source_fn=S.source, order_pens_fn=PD.order_pens_numpy)
    text = SC.tool_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(**kw), seam_fn=Seam(), improve_fn=Improve(), ring_entry_fn=never, **dbl)
    R, F, I = Rings(), Seam(), Improve()
    dbl.update(order_fn=never, order_pens_fn=never)                                          # the call stands in the place of both orders
    data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(ring_entry=True, **kw), seam_fn=F, improve_fn=I, ring_entry_fn=R, **dbl)
    st = info["ring_entry"]
    assert set(st) == set(RD.STAT_NAMES) and len(R.calls) == 1 and "ring_entry" not in pinfo
    off, pts, group, n_groups, reverse, (order, rev, seam, _) = R.calls[0]
    assert len(off) - 1 == info["paths"] == 30 and st["closed"] == 20 and st["moved"] >= 5 and n_groups == 1 and not group.any() and reverse == (mode == "all")
    assert st["candidates"] == int(np.where(np.diff(off) == 13, 12, np.where(np.diff(off) == 5, 4, 1 + reverse)).sum())
    rotated = R.entered()
    assert (rotated != pts).any() and st["travel"] == GC.travel_steps(*GC.gather_paths(off, rotated, order, rev))
    if I.calls:                                                                              # the improvement gets the ends of the rotated strokes, and the greedy sequence
        assert np.array_equal(I.calls[0][0], ends_of(off, rotated)) and np.array_equal(I.calls[0][1], order) and np.array_equal(I.calls[0][2], rev)
        assert info["improve"]["travel_before"] == st["travel"]
    if F.calls:                                                                              # the seam pass runs on the rotated strokes, behind the improvement
        assert np.array_equal(F.calls[0][0], off) and np.array_equal(F.calls[0][1], rotated)
        assert info["seam"]["travel_before"] == (info["improve"]["travel_after"] if I.calls else st["travel"])
    # pen-down steps are what they were: the streams differ by their pen-up steps alone
    last = lambda inf, t: inf["seam"]["travel_after"] if "seam" in inf else inf["improve"]["travel_after"] if "improve" in inf else t
    plain_order = D.order_numpy(ends_of(off, pts))
    plain_travel = GC.travel_steps(*GC.gather_paths(off, pts, plain_order)) if mode == "alone" else None
    assert info["steps"] - pinfo["steps"] == last(info, st["travel"]) - last(pinfo, plain_travel)
    assert st["travel"] < (plain_travel if mode == "alone" else pinfo["seam"]["travel_before"] if mode == "loop_start" else pinfo["improve"]["travel_before"])      # on this sheet it pays
    lines = list(GC.report_lines("gcode", info))
    assert GC.ring_entry_line("gcode", st) in lines and f"{st['closed']} closed strokes" in GC.ring_entry_line("gcode", st) and str(st["travel"]) in GC.ring_entry_line("gcode", st)
    assert not any("ring entry" in l for l in GC.report_lines("gcode", pinfo))


def test_a_result_that_breaks_the_rule_is_refused():
    from orip import gcode as GC
    text = SC.tool_gcode()

    def wrong(how):
        def fn(off, pts, group, n_groups, reverse):
            order, rev, seam, st = RD.order_rings(off, pts, group, n_groups, reverse)
            order, rev, seam, st = order.copy(), rev.copy(), seam.copy(), dict(st)
            lens = np.diff(off)[order]
            if how == "open": seam[int(np.nonzero(lens == 14)[0][0])] = 1                    # the circle with a tail is open
            if how == "range": seam[int(np.nonzero(lens == 5)[0][0])] = 4
            if how == "reversed_ring": rev[int(np.nonzero(lens == 5)[0][0])] = True
            if how == "reversed_open": rev[int(np.nonzero(lens == 14)[0][0])] = True           # without --allow-reverse
            if how == "twice": order[1] = order[0]
            if how == "count": st["moved"] += 1
            if how == "candidates": st["candidates"] -= 1
            if how == "travel": st["travel"] += 1
            if how == "short": seam = seam[:-1]
            return order, rev, seam, st
        return fn
    for how in ("open", "range", "reversed_ring", "reversed_open", "twice", "count", "candidates", "travel", "short"):
        with pytest.raises(RuntimeError):
            GC.build_stream_from_gcode(text, GC.GcodeOptions(ring_entry=True), ring_entry_fn=wrong(how), **GCODE_DOUBLES)


def test_svg_flow_with_pens_and_dots_of_one_point():
    from orip import svg as SV
    improve = lambda *a: ID.improve(*a[:6], (0, 0), a[6])
    for args, dbl in ((SC.TOOL_SVG_ARGS + ["--improve-order", "--loop-start"], lambda: dict(PD.pens_doubles(), improve_fn=improve)), ([], SVD.svg_doubles)):
        plain, pinfo = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(args), seam_fn=Seam(), ring_entry_fn=never, want_paths=True, **dbl())
        R, F = Rings(), Seam()
        data, info = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(args + ["--ring-entry"]), seam_fn=F, ring_entry_fn=R, want_paths=True,
                                              **dict(dbl(), order_fn=never, order_pens_fn=never))
        st = info["ring_entry"]
        assert len(R.calls) == 1 and st["closed"] == 12 and st["moved"] >= 1 and info["paths"] == pinfo["paths"] == 16
        assert R.calls[0][3] == (8 if args else 1) and R.calls[0][4] == bool(args)          # the pens are the groups; --allow-reverse is the flag
        if F.calls:
            assert np.array_equal(F.calls[0][1], R.entered())
        assert all(np.array_equal(a, b) for a, b in zip(info["fitted_paths"], pinfo["fitted_paths"]))       # the G-code file is what it was
        assert SV.GC.ring_entry_line("svg", st) in list(SV.GC.report_lines("svg", info))


def test_a_dot_is_an_open_stroke_of_one_point():
    from orip import svg as SV
    import stipple_cases as STC
    import test_stipple_host as TS
    Z, R, F = STC.StippleDouble(), Rings(), Seam()
    args = STC.TOOL_ARGS + TS.STIPPLE + ["--allow-reverse", "--ring-entry", "--loop-start"]
    data, info = SV.build_stream_from_svg(STC.TOOL_SVG, svg_options(args), **TS.doubles(Z, ring_entry_fn=R, seam_fn=F, order_fn=never, order_pens_fn=never))
    off, pts, group, n_groups, reverse, (order, rev, seam, st) = R.calls[0]
    dots = Z.out[2]["dots"]
    assert dots > 100 and (np.diff(off)[-dots:] == 1).all() and np.array_equal(pts[off[-1 - dots]:], Z.out[0]) and reverse
    assert info["ring_entry"]["candidates"] == st["candidates"] and st["closed"] == 3 and info["taps"] == dots == len(TS.taps_of(data))
    assert info["seam"]["travel_before"] == st["travel"]                                     # the seam pass is sent the rotated strokes, a dot as P, P
    rotated = R.entered()
    assert np.array_equal(F.calls[0][1][F.calls[0][0][:-1]], rotated[off[:-1]])


def test_tool_prints_the_report_line(tmp_path, capsys):
    from orip import gcode as GC
    src = tmp_path / "in.gcode"; src.write_text(SC.tool_gcode())
    GC.main([str(src), "-o", str(tmp_path / "out.bin"), "--ring-entry", "--loop-start"], seam_fn=Seam(), ring_entry_fn=Rings(), **GCODE_DOUBLES)
    out = capsys.readouterr().out
    assert "[gcode] ring entry: 20 closed strokes, " in out and "[gcode] loop start: 20 closed strokes" in out and out.index("ring entry") < out.index("loop start")
    with pytest.raises(ValueError, match="--ring-entry with --no-reorder"):
        GC.main([str(src), "-o", str(tmp_path / "out.bin"), "--ring-entry", "--no-reorder"], ring_entry_fn=never, **GCODE_DOUBLES)


def test_off_by_default_and_bytes_unchanged():
    from orip import gcode as GC, svg as SV
    text = SC.tool_gcode()
    for kw in ({}, dict(loop_start=True), dict(improve_order=True)):
        extra = dict(seam_fn=Seam(), improve_fn=Improve())
        a = GC.build_stream_from_gcode(text, GC.GcodeOptions(**kw), **extra, **GCODE_DOUBLES)
        b = GC.build_stream_from_gcode(text, GC.GcodeOptions(**kw), ring_entry_fn=never, **extra, **GCODE_DOUBLES)
        assert a[0] == b[0] and a[1] == b[1] and "ring_entry" not in b[1]
    a = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS), **PD.pens_doubles())
    b = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS), ring_entry_fn=never, **PD.pens_doubles())
    assert a[0] == b[0] and "ring_entry" not in b[1]
    from test_gcode_host import G, MAIN_CASES, options_for
    for i, (name, args) in enumerate(MAIN_CASES):                                            # the goldens of the tool as it was
        data, info = GC.build_stream_from_gcode(bytes(G[f"text_{name}"]), options_for(args), ring_entry_fn=never, **GCODE_DOUBLES)
        assert data == bytes(G[f"main_{i}_bin"]) and "ring_entry" not in info
