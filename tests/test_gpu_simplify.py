"""--simplify-mm on the GPU: orip_gcode_simplify against the sequential double of tests/simplify_double.py -- off, pts, kept, paths, points_in and points_out
-- on every shape of tests/simplify_cases.py; the resident form after a conversion and after a merge; every argument check, with the resident polylines left
as they were; and the whole tools, in process and as the scripts on disk, against the host flow run through the doubles and through the stage-14 decoder.
No comparison has a tolerance and no case is left out."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import simplify_cases as SC
import simplify_double as SD
import merge_cases as MC
import merge_double as MD
import gcode_double as D
import pens_double as PD
from stream_double import codes_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
TOP = 1 << 30
CASES = SC.cases()
MAP = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=1.0, W=4000, H=4000, invert_y=0)


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def equal(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int64
    for k, (a, b) in enumerate(zip(got[:3], want[:3])):
        assert a.shape == b.shape and np.array_equal(a, b), (k, a[:8], b[:8])
    assert {k: got[3][k] for k in ("paths", "points_in", "points_out")} == {k: want[3][k] for k in ("paths", "points_in", "points_out")}


# ------------------------------------------------------------------ the smallest shapes that can break the kernel
def test_nothing_to_simplify(dev):
    got = dev.gcode_simplify(np.zeros(1, np.int64), np.zeros((0, 2), np.int32), 4)
    equal(got, SD.simplify_numpy([0], np.zeros((0, 2)), 4))
    assert got[3]["rounds"] == 0
    off, pts = dev.gcode_steps_fetch(0, 0)
    assert off.tolist() == [0] and len(pts) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_shape(dev, name):
    off, pts, tol4 = CASES[name]
    want = SD.simplify_numpy(off, pts, tol4)
    got = dev.gcode_simplify(off, pts, tol4)
    equal(got, want)
    longest = int(np.diff(off).max())
    if longest <= SC.S:
        assert got[3]["rounds"] == 0                                          # every stroke was finished where it was first looked at
    if name == "walk":
        assert got[3]["rounds"] >= 2                                          # re-queued spans were re-queued again
    if name == f"local_{2 * SC.S + 3}":
        assert got[3]["rounds"] >= 1
    again = dev.gcode_simplify(None, None, tol4, n=len(off) - 1)              # the resident result once more: nothing changes
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1]) and np.array_equal(again[2], np.arange(len(want[1])))


def test_hand_worked_answers(dev):
    for pts, tol4, kept in SC.HAND:
        off, p = SC.strokes([[(x + SC.SHIFT, y + SC.SHIFT) for x, y in pts]])
        assert dev.gcode_simplify(off, p, tol4)[2].tolist() == kept
    for tol4, count in SC.STAIR_COUNTS.items():
        assert dev.gcode_simplify(*SC.strokes([SC.staircase()]), tol4)[3]["points_out"] == count


# ------------------------------------------------------------------ the resident form
def resident_input(dev):
    """a drawing in mm on a grid of one step per mm: a chain of three strokes along one line with a bend at its end, a stroke with points on a line, a lone
    stroke; one path the conversion drops"""
    lists = [[(5, 5), (9, 9)], [(9, 9), (20, 20)], [(30, 30), (30, 30.2)], [(20, 20), (26, 26), (26, 40)], [(40, 40), (45, 40), (50, 40), (50, 45), (50, 60)], [(70, 70), (80, 75)]]
    off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
    return dev.gcode_to_steps(off, np.asarray([q for p in lists for q in p], np.float64), MAP)


def ends_of(off, pts):
    return np.concatenate([pts[off[:-1]], pts[off[1:] - 1]], 1)


def test_resident_form_after_the_conversion(dev):
    off, pts = resident_input(dev)
    n = len(off) - 1
    assert n == 5 and dev.gcode_steps_source(n).tolist() == [0, 1, 3, 4, 5]
    want = SD.simplify_numpy(off, pts, 0)
    got = dev.gcode_simplify(None, None, 0, n=n)
    equal(got, want)
    assert want[3]["points_out"] == 2 + 2 + 3 + 3 + 2
    f_off, f_pts = dev.gcode_steps_fetch(n, want[3]["points_out"])
    assert np.array_equal(f_off, want[0]) and np.array_equal(f_pts, want[1])
    ends = ends_of(want[0], want[1])
    assert np.array_equal(ends, ends_of(off, pts))
    assert np.array_equal(dev.gcode_order(None, n=n), D.order_numpy(ends))
    o, r = dev.gcode_order_pens(None, np.zeros(n, np.int32), 1, True, n=n)
    wo, wr = PD.order_pens_numpy(ends, np.zeros(n, np.int32), 1, True)
    assert np.array_equal(o, wo) and np.array_equal(r, wr)
    assert dev.gcode_steps_source(n).tolist() == [0, 1, 3, 4, 5]              # the strokes are the same strokes


def test_resident_form_after_the_merge(dev):
    off, pts = resident_input(dev)
    n = len(off) - 1
    src = dev.gcode_steps_source(n)
    m_off, m_pts, moff, member, rev, mst = dev.gcode_merge(None, None, None, 1, False, n=n)
    assert mst["paths_out"] == 3 and np.array_equal(m_off, MD.merge_numpy(off, pts, None, 1, False)[0])
    want = SD.simplify_numpy(m_off, m_pts, 0)
    got = dev.gcode_simplify(None, None, 0, n=3)
    equal(got, want)
    assert np.diff(want[0]).tolist() == [3, 3, 2]                             # the joints inside the merged chain are gone: (5, 5) (26, 26) (26, 40)
    f_off, f_pts = dev.gcode_steps_fetch(3, 8)
    assert np.array_equal(f_off, want[0]) and np.array_equal(f_pts, want[1])
    assert np.array_equal(dev.gcode_order(None, n=3), D.order_numpy(ends_of(want[0], want[1])))
    resident_input(dev)
    assert np.array_equal(dev.gcode_steps_source(n), src)                     # and the next conversion names its sources again


# ------------------------------------------------------------------ bad arguments
def raw(dev, off, pts, n, tol4, stats=True):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = np.full(4, -7, np.int64)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((off, np.int64), (pts, np.int32))]
    rc = dev.L.orip_gcode_simplify(dev.h, p(keep[0]), p(keep[1]), int(n), int(tol4), p(st) if stats else None)
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def test_bad_arguments_leave_the_resident_paths(dev):
    off0, pts0 = resident_input(dev)
    n0, t0 = len(off0) - 1, len(pts0)
    o = np.array([0, 2, 5]); p = np.array([[1, 1], [2, 2], [2, 2], [3, 3], [9, 3]])
    bad = [("tol4 < 0", (o, p, 2, -1)), ("tol4 == 2^17", (o, p, 2, 1 << 17)), ("n < 0", (o, p, -1, 0)), ("n > 2^26", (o, p, (1 << 26) + 1, 0)),
           ("2^30 points", (np.array([0, 2, TOP]), p, 2, 0)), ("off[0] != 0", (np.array([1, 2, 5]), p, 2, 0)), ("off decreases", (np.array([0, 3, 2]), p, 2, 0)),
           ("a path of one point", (np.array([0, 4, 5]), p, 2, 0)), ("a path of no points", (np.array([0, 5, 5]), p, 2, 0)),
           ("x < 0", (o, np.array([[1, 1], [2, 2], [-1, 2], [3, 3], [9, 3]]), 2, 0)), ("y > 2^30", (o, np.array([[1, 1], [2, 2], [2, 2], [3, TOP + 1], [9, 3]]), 2, 0)),
           ("a point twice", (o, np.array([[1, 1], [2, 2], [2, 2], [3, 3], [3, 3]]), 2, 0)), ("a point twice", (np.array([0, 5]), p, 1, 0)),
           ("pts NULL", (o, None, 2, 0)), ("off NULL", (None, p, 2, 0)), ("not the resident count", (None, None, n0 + 1, 0)), ("not the resident count", (None, None, 0, 0))]
    for what, args in bad:
        rc, msg = raw(dev, *args)
        assert rc != 0 and "orip_gcode_simplify" in msg, what
    rc, msg = raw(dev, o, p, 2, 0, stats=False)
    assert rc != 0 and "orip_gcode_simplify" in msg
    off1, pts1 = dev.gcode_steps_fetch(n0, t0)
    assert np.array_equal(off1, off0) and np.array_equal(pts1, pts0) and len(dev.gcode_steps_source(n0)) == n0
    rc, msg = raw(dev, o, p, 2, 0)                                            # and the same arguments without a fault are taken
    assert rc == 0
    from orip.device import OripError
    for off, pts in ((o, None), (None, p)):
        with pytest.raises(OripError):
            dev.gcode_simplify(off, pts, 0)
    with pytest.raises(OripError):
        dev.gcode_simplify(o, p, 1 << 40)


# ------------------------------------------------------------------ the whole tools
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy, merge_fn=MD.merge_numpy, simplify_fn=SD.simplify_numpy)


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def run(script, args):
    return subprocess.run([sys.executable, os.path.join(SCRIPTS, script)] + args, capture_output=True, text=True, timeout=300)


def test_gcode_tool(dev, tmp_path):
    from orip import gcode as GC
    text = SC.tool_gcode()
    want, winfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(simplify_mm=SC.TOOL_MM), **GCODE_DOUBLES)
    got, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(simplify_mm=SC.TOOL_MM), dev)
    assert got == want and info["simplify"] == winfo["simplify"] and info["simplify"]["paths_changed"] == SC.LINE_STROKES + SC.CURVES - SC.COPIES
    (tmp_path / "drawing.gcode").write_text(text)
    r = run("gcode2stream.py", [str(tmp_path / "drawing.gcode"), "-o", str(tmp_path / "out.bin"), "--simplify-mm", str(SC.TOOL_MM)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = f"[gcode] simplify: {winfo['simplify']['points_in']} points -> {winfo['simplify']['points_out']} within 4 steps, {winfo['simplify']['paths_changed']} strokes changed"
    assert (tmp_path / "out.bin").read_bytes() == want and line in r.stdout
    for o in (GC.GcodeOptions(simplify_mm=0.05, merge_paths=True), GC.GcodeOptions(simplify_mm=0.05, merge_paths=True, allow_reverse=True), GC.GcodeOptions(simplify_mm=0.0, no_reorder=True)):
        S = PD.StepsWithSource()
        t2 = MC.tool_gcode() if o.merge_paths else text
        w2, wi = GC.build_stream_from_gcode(t2, o, **dict(GCODE_DOUBLES, steps_fn=S.steps, source_fn=S.source, order_pens_fn=PD.order_pens_numpy))
        g2, gi = GC.build_stream_from_gcode(t2, o, dev)
        assert g2 == w2 and gi["simplify"] == wi["simplify"] and gi["simplify"]["points_out"] < gi["simplify"]["points_in"]


def test_svg_tool_in_two_pens(dev, tmp_path):
    from orip import svg as SV
    dbl = dict(PD.pens_doubles(), simplify_fn=SD.simplify_numpy)
    want, winfo = SV.build_stream_from_svg(SC.tool_svg(), svg_options(SC.TOOL_SVG_ARGS), want_paths=True, **dbl)
    got, info = SV.build_stream_from_svg(SC.tool_svg(), svg_options(SC.TOOL_SVG_ARGS), dev, want_paths=True)
    assert got == want and info["simplify"] == winfo["simplify"] and info["simplify"]["points_out"] * 4 < info["simplify"]["points_in"] and info["pens"] == winfo["pens"]
    src = tmp_path / "drawing.svg"
    src.write_bytes(SC.tool_svg())
    r = run("svg2stream.py", [str(src), "--preview-render-width", "320", "--preview-render-height", "240"] + SC.TOOL_SVG_ARGS)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = f"[svg] simplify: {winfo['simplify']['points_in']} points -> {winfo['simplify']['points_out']} within 4 steps, {winfo['simplify']['paths_changed']} strokes changed"
    assert (tmp_path / "drawing_stream.bin").read_bytes() == want and line in r.stdout and (tmp_path / "drawing_stream_preview.png").exists()
    plain, pinfo = SV.build_stream_from_svg(SC.tool_svg(), svg_options(SC.TOOL_SVG_ARGS[2:]), want_paths=True, **PD.pens_doubles())
    assert (tmp_path / "drawing.gcode").read_text() == SV.gcode_text(*pinfo["fitted_paths"], pens=pinfo["path_pens"])      # the G-code file does not know of the pass


def test_tolerance_zero_draws_the_same(dev):
    """axis-aligned and 45-degree lines cut into pieces: without the vertices on the lines the pen makes the same steps, in fewer pieces and fewer bytes"""
    from orip import gcode as GC, stream_preview as SP
    text = SC.tool_gcode(curves=False)
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(), dev)
    thin, tinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(simplify_mm=0.0), dev)
    W, H = tinfo["target"]
    img_p, st_p = SP.preview(dev, plain, W, H, 320, 240, invert_y=True)
    img_t, st_t = SP.preview(dev, thin, W, H, 320, 240, invert_y=True)
    assert np.array_equal(img_p, img_t) and (img_t != 255).any()
    assert st_p["pen_down_segments"] == st_t["pen_down_segments"] == pinfo["paths"] == tinfo["paths"] == SC.LINE_STROKES
    down = lambda data: sum(len(s) - 1 for _, s in MC.strokes_of(data))
    assert down(plain) == down(thin) > 10000 and [s for _, s in MC.strokes_of(plain)] == [s for _, s in MC.strokes_of(thin)]
    assert tinfo["simplify"]["points_out"] == SC.LINE_CORNERS and tinfo["pieces"] < pinfo["pieces"] and tinfo["bytes"] < pinfo["bytes"] and len(thin) < len(plain)
    assert st_t["eof_seen"] == 1 and st_t["off_canvas_draws"] == 0 and st_t["steps_total"] == tinfo["steps"] == pinfo["steps"]
