"""--arcs on the GPU: orip_gcode_flatten against the sequential double of tests/arc_double.py, bit for bit (offsets, the float64 points as int64, the three
counts), on every named case of tests/arc_cases.py and the seeded random mixes; the hand-over of the resident polylines to orip_gcode_to_steps and
orip_gcode_to_steps_clip; every input the rule rejects, through the raw call, with nothing left resident and the context good afterwards; and gcode2stream
end to end, in process and as the script on disk.  No comparison has a tolerance.  Nothing here provokes a fault: the rejected inputs are values the
rule refuses by its own checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import arc_cases as AC
import arc_double as AD
import clip_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
CASES = dict(AC.small_cases(), **{f"random_{s}": AC.random_case(s) for s in AC.RANDOM_SEEDS})
_WANT = {}


def want(name):
    """the double's result, computed once"""
    if name not in _WANT:
        _WANT[name] = AD.flatten(CASES[name][:3], CASES[name][3])
    return _WANT[name]


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def flatten(dev, case):
    total, st = dev.gcode_flatten(case[:3], case[3])
    off, pts = dev.svg_paths()
    assert total == len(pts) == off[-1]
    return off, pts, st


# ------------------------------------------------------------------ against the double
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_double_bit_for_bit(dev, name):
    off, pts, st = flatten(dev, CASES[name])
    w_off, w_pts, w_st = want(name)
    assert off.dtype == np.int64 and pts.dtype == np.float64 and np.array_equal(off, w_off)
    assert pts.shape == w_pts.shape and np.array_equal(pts.view(np.int64), w_pts.view(np.int64)), np.flatnonzero((pts.view(np.int64) != w_pts.view(np.int64)).any(1))[:8]
    assert st == w_st


# ------------------------------------------------------------------ the hand-over
def test_the_resident_polylines_feed_the_conversion(dev):
    m = CC.sheet_map(4000, 4000, 20.0, offset_x_mm=100.0, offset_y_mm=100.0)
    for name in ("line_arc_line", "random_11", "block_of_segments"):
        w_off, w_pts, _ = want(name)
        up = dev.gcode_to_steps(w_off, w_pts, m)
        up_src = dev.gcode_steps_source(len(up[0]) - 1)
        flatten(dev, CASES[name])
        got = dev.gcode_to_steps(None, None, m, n=len(w_off) - 1)
        assert np.array_equal(got[0], up[0]) and np.array_equal(got[1], up[1]) and len(got[1]) > 10
        assert np.array_equal(dev.gcode_steps_source(len(got[0]) - 1), up_src)
    from orip.device import OripError
    with pytest.raises(OripError):
        dev.gcode_to_steps(None, None, m, n=len(w_off))                     # not the resident count


def test_the_resident_polylines_feed_the_clip(dev):
    """a circle half off the sheet, about a centre on the sheet's left edge, and a rounded corner inside it"""
    case = AC.table([[(AC.CW, (30.0, 50.0), (30.0, 50.0), (0.0, 50.0))], [(AC.LINE, (10.0, 10.0), (40.0, 10.0), None), (AC.CCW, (40.0, 10.0), (50.0, 20.0), (40.0, 20.0))]], 0.01)
    m = CC.sheet_map(2000, 2000, 20.0)
    w_off, w_pts, _ = AD.flatten(case[:3], case[3])
    for rect in ((0, 0, 1999, 1999), (100, 300, 1500, 1500)):
        up = dev.gcode_to_steps_clip(w_off, w_pts, m, rect)
        up_src = dev.gcode_steps_source(len(up[0]) - 1)
        flatten(dev, case)
        got = dev.gcode_to_steps_clip(None, None, m, rect, n=2)
        assert np.array_equal(got[0], up[0]) and np.array_equal(got[1], up[1]) and got[2] == up[2]
        assert got[2]["cut"] >= 2 and got[2]["outside"] > 10 and got[2]["inside"] > 10
        assert np.array_equal(dev.gcode_steps_source(len(got[0]) - 1), up_src)


# ------------------------------------------------------------------ what the rule rejects
def raw(dev, kind, seg, sub_off, tol, outs=(True, True)):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((kind, np.int32), (seg, np.float64), (sub_off, np.int64))]
    total, st = C.c_int64(-7), np.full(3, -7, np.int64)
    n_seg = 0 if keep[0] is None else len(keep[0])
    rc = dev.L.orip_gcode_flatten(dev.h, p(keep[0]), p(keep[1]), n_seg, p(keep[2]), 0 if keep[2] is None else len(keep[2]) - 1, float(tol), C.byref(total) if outs[0] else None,
                                  p(st) if outs[1] else None)
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode(), total.value


def test_rejected_inputs_leave_nothing_resident_and_the_context_good(dev):
    from orip.device import OripError
    k, s, o, tol = CASES["quarter_ccw"]
    one = np.array([0, 1])
    seg = lambda *v: np.array([v], np.float64)
    circles = 4096                                                          # full circles of depth 16: 2^18 pieces each, 2^30 in all
    many = (np.full(circles, 2), np.tile([1.0, 0.0, 1.0, 0.0, 0.0, 0.0], (circles, 1)), np.arange(circles + 1))
    bad = [("tol 0", (k, s, o, 0.0), "tolerance"), ("tol < 0", (k, s, o, -1.0), "tolerance"), ("tol inf", (k, s, o, float("inf")), "tolerance"),
           ("tol nan", (k, s, o, float("nan")), "tolerance"), ("kind 0", (np.array([0]), s, o, tol), "kind"), ("kind 4", (np.array([4]), s, o, tol), "kind"),
           ("centre nan", (k, seg(15, 10, 10, 15, float("nan"), 10), one, tol), "not finite"), ("start inf", (k, seg(float("inf"), 10, 10, 15, 10, 10), one, tol), "not finite"),
           ("line end nan", (np.array([1]), seg(0, 0, 1, float("nan"), 0, 0), one, tol), "not finite"), ("radius overflows", (k, seg(1e200, 0, 0, 1e200, 0, 0), one, tol), "not finite"),
           ("starts on its centre", (k, seg(15, 10, 10, 15, 15, 10), one, tol), "radius of 0"), ("ends on its centre", (k, seg(15, 10, 10, 15, 10, 15), one, tol), "radius of 0"),
           ("depth 17", (k, seg(1e9, 0, 0, 1e9, 0, 0), one, 1e-9), "2\\^18 pieces"), ("2^30 points", (*many, 1e-10), "points"),
           ("broken chain", (np.array([1, 1]), np.array([[0.0, 0, 1, 1, 0, 0], [1.0, 1.5, 2, 2, 0, 0]]), np.array([0, 2]), tol), "predecessor"),
           ("empty subpath", (np.array([1]), seg(0, 0, 1, 1, 0, 0), np.array([0, 0, 1]), tol), "no segment"), ("ranges", (np.array([1]), seg(0, 0, 1, 1, 0, 0), np.array([0, 2]), tol), "segment")]
    import re
    for what, args, msg in bad:
        flatten(dev, CASES["half_cw"])                                      # something resident for the call to take away
        rc, text, total = raw(dev, *args)
        assert rc != 0 and "orip_gcode_flatten" in text and re.search(msg, text) and total in (0, -7), (what, text)
        with pytest.raises(OripError, match="no paths"):
            dev.svg_paths(1)
        with pytest.raises(OripError):
            dev.gcode_to_steps(None, None, CC.sheet_map(100, 100, 1.0), n=1)
    for outs in ((False, True), (True, False)):
        rc, text, _ = raw(dev, k, s, o, tol, outs)
        assert rc != 0 and "orip_gcode_flatten" in text
    import hatch_double as HD
    assert dev.svg_flatten(HD.polys_table([[np.array([[1.0, 1.0], [9.0, 1.0], [5.0, 8.0]])]]), 1.0) == 3          # a later orip_svg_flatten on the same context
    off, pts = dev.gcode_to_steps(None, None, CC.sheet_map(100, 100, 1.0), n=1)
    assert pts.tolist() == [[1, 1], [9, 1], [5, 8]]
    off, pts, st = flatten(dev, CASES["quarter_cw"])                         # and a later orip_gcode_flatten
    assert np.array_equal(pts.view(np.int64), want("quarter_cw")[1].view(np.int64))
    rc, _, total = raw(dev, None, None, None, 0.1)                          # no segments: an empty list, resident
    assert rc == 0 and total == 0 and dev.svg_paths(0)[0].tolist() == [0]


# ------------------------------------------------------------------ the tool end to end
def doubles(**more):
    import clip_double as CD
    return dict(CD.gcode_doubles(), **more)


def test_gcode2stream_end_to_end(dev, tmp_path):
    from orip import gcode as GC, stream_preview as SP
    import merge_cases as MC
    tol = GC.arc_tolerance(GC.GcodeOptions(arcs=True))
    t, moves = GC.parse_gcode_arcs(AC.TOOL_GCODE)
    off, pts, wst = AD.flatten(t, tol)
    for kw in ({}, {"clip": True, "clip_margin_mm": 45.0}, {"allow_reverse": True, "merge_paths": True, "simplify_mm": 0.02}):
        fed, _ = GC.build_stream_from_gcode((off, pts), GC.GcodeOptions(**kw), **doubles(simplify_fn=_simplify()))
        got, info = GC.build_stream_from_gcode(AC.TOOL_GCODE, GC.GcodeOptions(arcs=True, **kw), dev)
        assert got == fed and info["arcs"] == dict(wst, tolerance_mm=tol) and info["pen_down_moves"] == moves
    arcs, ainfo = GC.build_stream_from_gcode(AC.TOOL_GCODE, GC.GcodeOptions(arcs=True), dev)
    chords, cinfo = GC.build_stream_from_gcode(AC.TOOL_GCODE, GC.GcodeOptions(), dev)
    W, H = ainfo["target"]
    ast, cst = (SP.preview(dev, d, W, H, 320, 240, invert_y=True)[1] for d in (arcs, chords))
    assert ast["pen_down_segments"] == cst["pen_down_segments"] == 2 and ast["eof_seen"] == 1 and ast["off_canvas_draws"] == 0      # the same strokes,
    assert ast["steps_total"] == ainfo["steps"] > cst["steps_total"]
    a, c = MC.strokes_of(arcs), MC.strokes_of(chords)
    assert len(a) == len(c) == 2 and sum(len(p) - 1 for _, p in a) > sum(len(p) - 1 for _, p in c)                                 # and more pen-down steps
    assert GC.build_stream_from_gcode(CC.circle_gcode(), GC.GcodeOptions(arcs=True), dev)[0] == GC.build_stream_from_gcode(CC.circle_gcode(), GC.GcodeOptions(), dev)[0]
    src = tmp_path / "drawing.gcode"
    src.write_text(AC.TOOL_GCODE)
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "gcode2stream.py"), str(src), "-o", str(tmp_path / "out.bin"), "--arcs"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "out.bin").read_bytes() == arcs
    assert f"[gcode] arcs: 6 arcs drawn in {wst['pieces']} pieces within 0.0125 mm, 0 full circles" in r.stdout


def _simplify():
    import simplify_double as SP
    return SP.simplify_numpy


def test_a_circle_is_a_closed_stroke_for_ring_entry_and_loop_start(dev):
    from orip import gcode as GC
    o = dict(loop_start=True, ring_entry=True)
    _, ainfo = GC.build_stream_from_gcode(AC.TOOL_GCODE, GC.GcodeOptions(arcs=True, **o), dev)
    _, cinfo = GC.build_stream_from_gcode(AC.TOOL_GCODE, GC.GcodeOptions(**o), dev)
    assert ainfo["ring_entry"]["closed"] == ainfo["seam"]["closed"] == 2    # the circle of two halves and the rounded rectangle: first point == last point after conversion
    assert cinfo["ring_entry"]["closed"] == 1                               # as chords the circle is a diameter drawn there and back: three points, no ring
    t, _ = GC.parse_gcode_arcs(AC.TOOL_GCODE)
    dev.gcode_flatten(t, GC.arc_tolerance(GC.GcodeOptions(arcs=True)))
    off, pts = dev.gcode_to_steps(None, None, dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=40.0, W=8400, H=11880, invert_y=0), n=2)
    for p in range(2):
        assert off[p + 1] - off[p] >= 4 and pts[off[p]].tolist() == pts[off[p + 1] - 1].tolist()
