"""--dedup on the GPU: orip_gcode_dedup against the sequential double of tests/dedup_double.py -- off, pts, origin and all nine stats -- on every named drawing
of tests/dedup_cases.py and on random drawings; the resident form behind the conversion, behind the clip and in front of the merge; the uploaded form with
and without a resident list, and what the sources say then; every argument check, with the resident polylines left as they were; idempotence; and the whole
tools against the host flow run through the doubles and through the stage-14 decoder.  No comparison has a tolerance and no case is left out."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dedup_cases as DC
import dedup_double as DD
import merge_double as MD
import gcode_double as D
import pens_double as PD
from stream_double import codes_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
TOP = 1 << 30
CASES = DC.cases()
MAP = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=1.0, W=4000, H=4000, invert_y=0)


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def equal(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    for k, (a, b) in enumerate(zip(got[:3], want[:3])):
        assert a.shape == b.shape and np.array_equal(a, b), (k, a[:8], b[:8])
    assert got[3] == want[3]


# ------------------------------------------------------------------ every drawing against the double
def test_nothing_to_dedup(dev):
    got = dev.gcode_dedup(np.zeros(1, np.int64), np.zeros((0, 2), np.int32), None, 1)
    equal(got, DD.dedup_numpy([0], np.zeros((0, 2)), None, 1))
    off, pts = dev.gcode_steps_fetch(0, 0)
    assert off.tolist() == [0] and len(pts) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_shape(dev, name):
    off, pts, group, n_groups = CASES[name]
    want = DD.dedup_numpy(off, pts, group, n_groups)
    got = dev.gcode_dedup(off, pts, group, n_groups)
    equal(got, want)
    f_off, f_pts = dev.gcode_steps_fetch(len(want[0]) - 1, len(want[1]))
    assert np.array_equal(f_off, want[0]) and np.array_equal(f_pts, want[1])
    g2 = None if group is None else group[want[2]]
    again = dev.gcode_dedup(None, None, g2, n_groups, n=len(want[0]) - 1)      # the resident result once more: nothing changes
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1]) and np.array_equal(again[2], np.arange(len(want[0]) - 1))
    assert again[3]["whole"] == again[3]["segments"] == want[3]["pieces"] and again[3]["draw_steps_in"] == again[3]["draw_steps_out"] == want[3]["draw_steps_out"]


def test_hand_worked_answers(dev):
    for lists, groups, out, origin in DC.HAND:
        off, pts = DC.strokes(lists)
        got = dev.gcode_dedup(off, pts, groups, 2)
        w_off, w_pts = DC.strokes(out)
        assert np.array_equal(got[0], w_off) and np.array_equal(got[1], w_pts) and got[2].tolist() == origin


def test_random_drawings(dev):
    for seed in range(300):
        off, pts, group, n_groups = DC.random_drawing(seed)
        equal(dev.gcode_dedup(off, pts, group, n_groups), DD.dedup_numpy(off, pts, group, n_groups))


def test_many_random_strokes_in_one_call(dev):
    """the random drawings side by side in one call, shifted apart: more than one block, lines of every length next to each other"""
    lists, groups = [], []
    for seed in range(400):
        off, pts, group, _ = DC.random_drawing(seed)
        lists += [[(x + 10 * (seed % 20), y + 10 * (seed // 20)) for x, y in pts[a:b].tolist()] for a, b in zip(off[:-1], off[1:])]
        groups += group.tolist()
    off, pts = DC.strokes(lists)
    equal(dev.gcode_dedup(off, pts, np.asarray(groups, np.int32), 2), DD.dedup_numpy(off, pts, groups, 2))


# ------------------------------------------------------------------ the resident form
def resident_input(dev, clip=None):
    """a drawing in mm on a grid of one step per mm: two squares that share an edge, a path the conversion drops, a stroke out and back, one over the squares' top"""
    lists = [DC.square(10, 10, 20), [(50, 50), (50, 50.2)], DC.square(30, 10, 20), [(5, 60), (45, 60), (25, 60)], [(0, 10), (60, 10)]]
    off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
    mm = np.asarray([q for p in lists for q in p], np.float64)
    if clip is None:
        return dev.gcode_to_steps(off, mm, MAP)
    return dev.gcode_to_steps_clip(off, mm, MAP, clip)[:2]


def test_resident_form_after_the_conversion_and_before_the_merge(dev):
    off, pts = resident_input(dev)
    n = len(off) - 1
    src = dev.gcode_steps_source(n)
    assert n == 4 and src.tolist() == [0, 2, 3, 4]
    want = DD.dedup_numpy(off, pts, None, 1)
    got = dev.gcode_dedup(None, None, None, 1, n=n)
    equal(got, want)
    assert want[3]["covered"] == 2 and want[3]["cut"] == 1 and want[2].tolist() == [0, 1, 2, 3, 3]
    k = len(want[0]) - 1
    f_off, f_pts = dev.gcode_steps_fetch(k, len(want[1]))
    assert np.array_equal(f_off, want[0]) and np.array_equal(f_pts, want[1])
    assert dev.gcode_steps_source(k).tolist() == src[want[2]].tolist() == [0, 2, 3, 4, 4]      # the input path of every stroke, gathered through origin
    assert np.array_equal(dev.gcode_order(None, n=k), D.order_numpy(np.concatenate([want[1][want[0][:-1]], want[1][want[0][1:] - 1]], 1)))
    m = dev.gcode_merge(None, None, None, 1, True, n=k)                       # the pieces are what the merge joins
    wm = MD.merge_numpy(want[0], want[1], None, 1, True)
    assert np.array_equal(m[0], wm[0]) and np.array_equal(m[1], wm[1]) and m[5]["joins"] == wm[5]["joins"]
    from orip.device import OripError
    with pytest.raises(OripError):
        dev.gcode_steps_source(len(m[0]) - 1)                                 # merged: the sources no longer name the strokes


def test_resident_form_after_the_clip(dev):
    off, pts = resident_input(dev, clip=(0, 0, 40, 3999))                     # the second square and the long strokes are cut at x = 40
    n = len(off) - 1
    src = dev.gcode_steps_source(n)
    assert len(set(src.tolist())) < n                                         # sources with repeats
    want = DD.dedup_numpy(off, pts, None, 1)
    got = dev.gcode_dedup(None, None, None, 1, n=n)
    equal(got, want)
    assert want[3]["covered"] >= 2
    assert dev.gcode_steps_source(len(want[0]) - 1).tolist() == src[want[2]].tolist()


def drop_the_list(dev):
    rc = dev.L.orip_gcode_to_steps(dev.h, None, None, 0, None, None, None)     # the conversion drops the list before it looks at its arguments
    assert rc != 0
    with pytest.raises(Exception):
        dev.gcode_steps_fetch(0, 0)


def test_uploaded_form_and_the_sources(dev):
    from orip.device import OripError
    name = "long_first_then_shorts"
    off, pts, group, n_groups = CASES[name]
    want = DD.dedup_numpy(off, pts, group, n_groups)
    drop_the_list(dev)
    equal(dev.gcode_dedup(off, pts, group, n_groups), want)                   # no list resident: the strokes have no sources
    with pytest.raises(OripError):
        dev.gcode_steps_source(len(want[0]) - 1)
    r_off, r_pts = resident_input(dev)                                        # 4 strokes resident, as many as the case has: taken for the polylines a fetch gave out
    assert len(r_off) - 1 == len(off) - 1 == 4
    src = dev.gcode_steps_source(4)
    equal(dev.gcode_dedup(off, pts, group, n_groups), want)
    assert dev.gcode_steps_source(len(want[0]) - 1).tolist() == src[want[2]].tolist() == [0, 3, 4]
    resident_input(dev)
    o2, p2, g2, n2 = CASES["two_squares"]                                     # another count: the sources do not name these
    equal(dev.gcode_dedup(o2, p2, g2, n2), DD.dedup_numpy(o2, p2, g2, n2))
    with pytest.raises(OripError):
        dev.gcode_steps_source(2)
    resident_input(dev)
    assert dev.gcode_steps_source(4).tolist() == [0, 2, 3, 4]                 # and the next conversion names its sources again


# ------------------------------------------------------------------ bad arguments
def raw(dev, off, pts, group, n, n_groups, stats=True):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = np.full(9, -7, np.int64)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((off, np.int64), (pts, np.int32), (group, np.int32))]
    rc = dev.L.orip_gcode_dedup(dev.h, p(keep[0]), p(keep[1]), p(keep[2]), int(n), int(n_groups), p(st) if stats else None)
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def test_bad_arguments_leave_the_resident_paths(dev):
    off0, pts0 = resident_input(dev)
    n0, t0 = len(off0) - 1, len(pts0)
    src0 = dev.gcode_steps_source(n0)
    o = np.array([0, 2, 5]); p = np.array([[1, 1], [2, 2], [2, 2], [3, 3], [9, 3]]); g = np.array([0, 1])
    bad = [("n < 0", (o, p, g, -1, 2)), ("n > 2^26", (o, p, g, (1 << 26) + 1, 2)), ("2^28 points", (np.array([0, 2, 1 << 28]), p, g, 2, 2)),
           ("off[0] != 0", (np.array([1, 2, 5]), p, g, 2, 2)), ("off decreases", (np.array([0, 3, 2]), p, g, 2, 2)),
           ("a path of one point", (np.array([0, 4, 5]), p, g, 2, 2)), ("a path of no points", (np.array([0, 5, 5]), p, g, 2, 2)),
           ("x < 0", (o, np.array([[1, 1], [2, 2], [-1, 2], [3, 3], [9, 3]]), g, 2, 2)), ("y > 2^30", (o, np.array([[1, 1], [2, 2], [2, 2], [3, TOP + 1], [9, 3]]), g, 2, 2)),
           ("a point twice", (o, np.array([[1, 1], [2, 2], [2, 2], [3, 3], [3, 3]]), g, 2, 2)), ("a point twice", (np.array([0, 5]), p, None, 1, 1)),
           ("group < 0", (o, p, np.array([0, -1]), 2, 2)), ("group == n_groups", (o, p, np.array([0, 2]), 2, 2)), ("n_groups 0", (o, p, None, 2, 0)), ("n_groups 65", (o, p, g, 2, 65)),
           ("pts NULL", (o, None, g, 2, 2)), ("off NULL", (None, p, g, 2, 2)), ("not the resident count", (None, None, None, n0 + 1, 1)), ("not the resident count", (None, None, None, 0, 1))]
    for what, args in bad:
        rc, msg = raw(dev, *args)
        assert rc != 0 and "orip_gcode_dedup" in msg, what
    rc, msg = raw(dev, o, p, g, 2, 2, stats=False)
    assert rc != 0 and "orip_gcode_dedup" in msg
    off1, pts1 = dev.gcode_steps_fetch(n0, t0)
    assert np.array_equal(off1, off0) and np.array_equal(pts1, pts0) and np.array_equal(dev.gcode_steps_source(n0), src0)
    rc, msg = raw(dev, o, p, g, 2, 2)                                         # and the same arguments without a fault are taken
    assert rc == 0
    from orip.device import OripError
    for off, pts in ((o, None), (None, p)):
        with pytest.raises(OripError):
            dev.gcode_dedup(off, pts, None, 1)
    with pytest.raises(OripError):
        dev.gcode_dedup(None, None, None, 1, n=3)
    with pytest.raises(OripError):
        dev._ck(dev.L.orip_gcode_dedup_fetch(dev.h, None))                    # a result of two strokes and nowhere to put it


# ------------------------------------------------------------------ the whole tools
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy, merge_fn=MD.merge_numpy, dedup_fn=DD.dedup_numpy)


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def run(script, args):
    return subprocess.run([sys.executable, os.path.join(SCRIPTS, script)] + args, capture_output=True, text=True, timeout=300)


def test_gcode_tool(dev, tmp_path):
    from orip import gcode as GC
    text = DC.tool_gcode()
    for o in (GC.GcodeOptions(dedup=True), GC.GcodeOptions(dedup=True, merge_paths=True), GC.GcodeOptions(dedup=True, no_reorder=True)):
        want, winfo = GC.build_stream_from_gcode(text, o, **GCODE_DOUBLES)
        got, info = GC.build_stream_from_gcode(text, o, dev)
        assert got == want and info["dedup"] == winfo["dedup"] and info.get("merge") == winfo.get("merge") and info["paths"] == winfo["paths"]
        assert (info["dedup"]["draw_steps_in"], info["dedup"]["draw_steps_out"]) == (DC.GRID_STEPS_IN, DC.GRID_STEPS_OUT)
    S = PD.StepsWithSource()
    o = GC.GcodeOptions(dedup=True, merge_paths=True, allow_reverse=True, simplify_mm=0.0)
    want, winfo = GC.build_stream_from_gcode(text, o, **dict(GCODE_DOUBLES, steps_fn=S.steps, source_fn=S.source, order_pens_fn=PD.order_pens_numpy,
                                                              simplify_fn=__import__("simplify_double").simplify_numpy))
    got, info = GC.build_stream_from_gcode(text, o, dev)
    assert got == want and info["dedup"] == winfo["dedup"] and info["merge"] == winfo["merge"] and info["simplify"] == winfo["simplify"] and info["paths"] < 9
    (tmp_path / "grid.gcode").write_text(text)
    want, winfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(dedup=True, merge_paths=True), **GCODE_DOUBLES)
    r = run("gcode2stream.py", [str(tmp_path / "grid.gcode"), "-o", str(tmp_path / "out.bin"), "--dedup", "--merge-paths"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = f"[gcode] dedup: 36 segments: 24 whole, 0 cut, 12 covered -> 9 strokes, pen-down steps {DC.GRID_STEPS_IN} -> {DC.GRID_STEPS_OUT}"
    assert (tmp_path / "out.bin").read_bytes() == want and line in r.stdout


def test_svg_tool_in_two_pens(dev, tmp_path):
    from orip import svg as SV
    dbl = dict(PD.pens_doubles(), dedup_fn=DD.dedup_numpy)
    want, winfo = SV.build_stream_from_svg(DC.tool_svg(), svg_options(DC.TOOL_SVG_ARGS), want_paths=True, **dbl)
    got, info = SV.build_stream_from_svg(DC.tool_svg(), svg_options(DC.TOOL_SVG_ARGS), dev, want_paths=True)
    assert got == want and info["dedup"] == winfo["dedup"] and info["pens"] == winfo["pens"]
    d = info["dedup"]
    assert d["segments"] == 16 and d["covered"] == 2 and d["whole"] == 14 and d["draw_steps_in"] - d["draw_steps_out"] == 2 * 20 * 40      # one border per pen; the one across stays
    src = tmp_path / "drawing.svg"
    src.write_bytes(DC.tool_svg())
    r = run("svg2stream.py", [str(src), "--preview-render-width", "320", "--preview-render-height", "240"] + DC.TOOL_SVG_ARGS)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = f"[svg] dedup: 16 segments: 14 whole, 0 cut, 2 covered -> {d['paths_out']} strokes, pen-down steps {d['draw_steps_in']} -> {d['draw_steps_out']}"
    assert (tmp_path / "drawing_stream.bin").read_bytes() == want and line in r.stdout and (tmp_path / "drawing_stream_preview.png").exists()
    plain, pinfo = SV.build_stream_from_svg(DC.tool_svg(), svg_options(DC.TOOL_SVG_ARGS[1:]), want_paths=True, **PD.pens_doubles())
    assert (tmp_path / "drawing.gcode").read_text() == SV.gcode_text(*pinfo["fitted_paths"], pens=pinfo["path_pens"])      # the G-code file does not know of the pass


def test_the_stream_inks_the_same_pixels(dev):
    """the stream with --dedup replays in 14_preview_stream to the same inked pixels as without it.  The preview draws a pixel dark however often the pen
    passes, so the images could be compared whole; the non-background mask is what the rule promises, and it is what is compared"""
    from orip import gcode as GC, stream_preview as SP
    text = DC.tool_gcode()
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(), dev)
    once, oinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(dedup=True), dev)
    W, H = oinfo["target"]
    img_p, st_p = SP.preview(dev, plain, W, H, 420, 594, invert_y=True)
    img_o, st_o = SP.preview(dev, once, W, H, 420, 594, invert_y=True)
    ink = lambda img: (np.asarray(img).reshape(img.shape[0], img.shape[1], -1) != 255).any(2)
    assert np.array_equal(ink(img_p), ink(img_o)) and ink(img_o).any()
    assert st_o["eof_seen"] == 1 and st_o["off_canvas_draws"] == 0 and len(once) < len(plain)
