"""--clip on the GPU: orip_gcode_to_steps_clip against the sequential double of tests/clip_double.py in all four outputs (offsets, points, sources, counts),
on every crafted shape of tests/clip_cases.py by name and on the random drawing; the resident SVG form; what is resident afterwards, through the fetches,
the order and the merge; every argument check through the raw call, with the resident polylines left as they were; both tools, in process and as the
scripts on disk, byte for byte against the host flow through the doubles; and the preview of a drawing half off the sheet.  No comparison has a tolerance
and no case is left out."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import clip_cases as CC
import clip_double as CD
import gcode_double as D
import merge_double as MD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
TOP = 1 << 30
SMALL = CC.small_cases()


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def clip(dev, case):
    """the device's four outputs"""
    off, pts, st = dev.gcode_to_steps_clip(*case)
    return off, pts, dev.gcode_steps_source(len(off) - 1), st


def equal(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    for k, (a, b) in enumerate(zip(got[:3], want[:3])):
        assert a.shape == b.shape and np.array_equal(a, b), (k, a[:8], b[:8])
    assert got[3] == want[3]


# ------------------------------------------------------------------ against the double
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_shape(dev, name):
    equal(clip(dev, SMALL[name]), CD.clip_numpy(*SMALL[name]))


@pytest.fixture(scope="module")
def random_case():
    case = CC.random_case()
    return case, CD.clip_numpy(*case)


def test_random_case(dev, random_case):
    case, want = random_case
    equal(clip(dev, case), want)
    assert want[3]["inside"] > 100 and want[3]["cut"] > 100 and want[3]["outside"] > 100


def test_range_and_finite_errors_leave_nothing_resident(dev):
    from orip.device import OripError
    clip(dev, SMALL["path_zigzag"])
    with pytest.raises(OripError, match="off the sheet"):
        dev.gcode_to_steps_clip(*CC.range_error_case())
    with pytest.raises(OripError):
        dev.gcode_steps_fetch(1, 2)
    with pytest.raises(OripError, match="not finite"):
        dev.gcode_to_steps_clip(*CC.case([[(1, 1), (float("inf"), 2)]]))
    equal(clip(dev, CC.case([[(1, 1), (2, 2)], [(float("nan"), 2)], [(TOP + 5, 0)]])), CD.clip_numpy(*CC.case([[(1, 1), (2, 2)], [(float("nan"), 2)], [(TOP + 5, 0)]])))      # lone points are not looked at
    ok = CC.case([[(1, 1), (TOP, -TOP)]])                                  # 2^30 itself is inside the range
    equal(clip(dev, ok), CD.clip_numpy(*ok))


# ------------------------------------------------------------------ the resident SVG form
def test_resident_svg_form(dev):
    from orip import svg as SV
    o = SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg"] + CC.TOOL_SVG_ARGS))
    table = SV.parse_svg(CC.TOOL_SVG)
    R = SV._Resident(dev)
    paths, _ = SV.fit_paths(table, o, R.flatten, R.bbox, R.fit)
    off_mm, pts_mm = R.fetch(paths, True)
    m = CC.sheet_map(1000, 1000, 10.0)
    for rect in ((0, 0, 999, 999), (25, 40, 900, 700)):
        want = CD.clip_numpy(off_mm, pts_mm, m, rect)
        off, pts, st = R.clip(paths, m, rect)
        equal((off, pts, R.source(len(off) - 1), st), want)
        assert want[3]["cut"] >= 5 and want[3]["outside"] >= 4 and want[3]["inside"] >= 10         # 72 segments; 23 / 8 / 41 on the sheet, 11 / 7 / 54 in the smaller rectangle
    from orip.device import OripError
    with pytest.raises(OripError):
        dev.gcode_to_steps_clip(None, None, m, (0, 0, 999, 999), n=paths["n"] + 1)      # not the resident count


# ------------------------------------------------------------------ what is resident afterwards
def test_resident_strokes_feed_the_later_steps(dev, random_case):
    import pens_double as PD
    case, want = random_case
    off, pts, st = dev.gcode_to_steps_clip(*case)
    n, total = len(off) - 1, len(pts)
    f_off, f_pts = dev.gcode_steps_fetch(n, total)
    assert np.array_equal(f_off, want[0]) and np.array_equal(f_pts, want[1]) and np.array_equal(dev.gcode_steps_source(n), want[2])
    ends = np.concatenate([want[1][want[0][:-1]], want[1][want[0][1:] - 1]], 1)
    assert np.array_equal(dev.gcode_order(None, n=n), D.order_numpy(ends))
    grp = (want[2] % 3).astype(np.int32)
    o, r = dev.gcode_order_pens(None, grp, 3, True, n=n)
    wo, wr = PD.order_pens_numpy(ends, grp, 3, True)
    assert np.array_equal(o, wo) and np.array_equal(r, wr)
    got = dev.gcode_merge(None, None, None, 1, True, n=n)
    wm = MD.merge_numpy(want[0], want[1], None, 1, True)
    for a, b in zip(got[:5], wm[:5]):
        assert np.array_equal(a, b)
    assert got[5] == wm[5] and wm[5]["joins"] > 0                          # the merge has something to join: strokes that share a border point (6 joins by the double)
    off2, pts2, _ = dev.gcode_to_steps_clip(*case)                         # the next clip names its sources again
    assert np.array_equal(dev.gcode_steps_source(len(off2) - 1), want[2])
    s_off, s_pts = dev.gcode_to_steps(case[0], case[1], case[2])           # and the plain conversion is what it was
    w_off, w_pts = D.to_steps_numpy(case[0], case[1], case[2])
    assert np.array_equal(s_off, w_off) and np.array_equal(s_pts, w_pts)


# ------------------------------------------------------------------ bad arguments
def raw(dev, off, pts, n, m, rect, outs=(True, True, True)):
    from orip import lib
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((off, np.int64), (pts, np.float64), (rect, np.int32))]
    gm = None if m is None else lib.GcodeMap(**m)
    n_out, tot, st = C.c_int64(-7), C.c_int64(-7), np.full(6, -7, np.int64)
    rc = dev.L.orip_gcode_to_steps_clip(dev.h, p(keep[0]), p(keep[1]), int(n), None if gm is None else C.byref(gm), p(keep[2]), C.byref(n_out) if outs[0] else None,
                                        C.byref(tot) if outs[1] else None, p(st) if outs[2] else None)
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def test_bad_arguments_leave_the_resident_paths(dev):
    off0, pts0, src0, _ = clip(dev, SMALL["path_zigzag"])
    n0, t0 = len(off0) - 1, len(pts0)
    o = np.array([0, 2, 4]); p = np.array([[1.0, 1], [9, 2], [2, 2], [3, 3]]); m = CC.sheet_map(); r = np.array([0, 0, 7, 7])
    bad = [("n < 0", (o, p, -1, m, r)), ("2^30 paths", (o, p, TOP, m, r)), ("2^29 points", (np.array([0, 2, 1 << 29]), p, 2, m, r)), ("off[0] != 0", (np.array([1, 2, 4]), p, 2, m, r)),
           ("off decreases", (np.array([0, 3, 2]), p, 2, m, r)), ("pts NULL", (o, None, 2, m, r)), ("off NULL", (None, p, 2, m, r)), ("map NULL", (o, p, 2, None, r)),
           ("W = 0", (o, p, 2, dict(m, W=0), np.array([0, 0, 0, 7]))), ("H > 2^30", (o, p, 2, dict(m, H=TOP + 1), r)), ("rect NULL", (o, p, 2, m, None)),
           ("x0 > x1", (o, p, 2, m, np.array([5, 0, 4, 7]))), ("y0 > y1", (o, p, 2, m, np.array([0, 7, 7, 6]))), ("x0 < 0", (o, p, 2, m, np.array([-1, 0, 7, 7]))),
           ("y0 < 0", (o, p, 2, m, np.array([0, -1, 7, 7]))), ("x1 > W - 1", (o, p, 2, m, np.array([0, 0, 8, 7]))), ("y1 > H - 1", (o, p, 2, m, np.array([0, 0, 7, 8]))),
           ("no fitted paths of that count", (None, None, 1 << 20, m, r))]
    for what, args in bad:
        rc, msg = raw(dev, *args)
        assert rc != 0 and "orip_gcode_to_steps_clip" in msg, what
    for outs in ((False, True, True), (True, False, True), (True, True, False)):
        rc, msg = raw(dev, o, p, 2, m, r, outs)
        assert rc != 0 and "orip_gcode_to_steps_clip" in msg, outs
    off1, pts1 = dev.gcode_steps_fetch(n0, t0)
    assert np.array_equal(off1, off0) and np.array_equal(pts1, pts0) and np.array_equal(dev.gcode_steps_source(n0), src0)
    rc, msg = raw(dev, o, p, 2, m, r)                                      # and the same call with good arguments is taken
    assert rc == 0
    f_off, f_pts = dev.gcode_steps_fetch(2, 4)
    assert f_off.tolist() == [0, 2, 4] and f_pts.tolist() == [[1, 1], [7, 2], [2, 2], [3, 3]]
    from orip.device import OripError
    with pytest.raises(OripError):
        dev.gcode_to_steps_clip(o, p, m, (0, 0, 7))


# ------------------------------------------------------------------ the whole tools
def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def run(script, args):
    return subprocess.run([sys.executable, os.path.join(SCRIPTS, script)] + args, capture_output=True, text=True, timeout=300)


def test_gcode_tool(dev, tmp_path):
    from orip import gcode as GC
    text = CC.circle_gcode()
    want, winfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(clip=True), **CD.gcode_doubles())
    got, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(clip=True), dev)
    assert got == want and info["clip"] == winfo["clip"] and info["clip"]["cut"] == 2 and info["clip"]["paths_out"] == 3
    (tmp_path / "drawing.gcode").write_text(text)
    r = run("gcode2stream.py", [str(tmp_path / "drawing.gcode"), "-o", str(tmp_path / "out.bin"), "--clip"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "out.bin").read_bytes() == want and "[gcode] clip: 94 segments: " in r.stdout and "-> 3 strokes" in r.stdout
    for o in (GC.GcodeOptions(clip=True, clip_margin_mm=5.0, no_reorder=True), GC.GcodeOptions(clip=True, allow_reverse=True, merge_paths=True, improve_order=True)):
        assert GC.build_stream_from_gcode(text, o, dev)[0] == GC.build_stream_from_gcode(text, o, **CD.gcode_doubles())[0]
    plain = GC.build_stream_from_gcode(CC.inside_gcode(), GC.GcodeOptions(tool_pens=True), dev)
    clipped = GC.build_stream_from_gcode(CC.inside_gcode(), GC.GcodeOptions(tool_pens=True, clip=True), dev)
    assert plain[0] == clipped[0] and clipped[1]["clip"]["cut"] == clipped[1]["clip"]["outside"] == 0      # on the sheet the option changes nothing


def test_svg_tool_with_pens_and_hatch(dev, tmp_path):
    from orip import svg as SV
    args = CC.TOOL_SVG_ARGS + ["--pen-colors", "#f00,#0f0,#00f", "--hatch-spacing-mm", "2.0", "--hatch-inset-mm", "0", "--merge-paths"]
    want, winfo = SV.build_stream_from_svg(CC.TOOL_SVG, svg_options(args), want_paths=True, **CD.svg_doubles())
    got, info = SV.build_stream_from_svg(CC.TOOL_SVG, svg_options(args), dev, want_paths=True)
    assert got == want and info["clip"] == winfo["clip"] and info["pens"] == winfo["pens"] and info["merge"] == winfo["merge"] and info["clip"]["cut"] >= 20
    src = tmp_path / "drawing.svg"
    src.write_bytes(CC.TOOL_SVG)
    r = run("svg2stream.py", [str(src), "--preview-render-width", "400", "--preview-render-height", "400"] + args)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "drawing_stream.bin").read_bytes() == want and "[svg] clip: " in r.stdout and (tmp_path / "drawing_stream_preview.png").exists()
    assert "-> %d strokes" % info["clip"]["paths_out"] in r.stdout
    plain, pinfo = SV.build_stream_from_svg(CC.TOOL_SVG, svg_options([a for a in args if a != "--clip"]), want_paths=True, **CD.svg_doubles())
    assert (tmp_path / "drawing.gcode").read_text() == SV.gcode_text(*pinfo["fitted_paths"], pens=pinfo["path_pens"])      # the G-code file does not know of the clip


# ------------------------------------------------------------------ the preview
def test_preview_of_a_drawing_half_off_the_sheet(dev):
    """one step to the pixel: the clamp inks the border column from the circle's lowest to its highest point; the clip leaves the two pixels where the arcs end,
    and with a margin nothing at all"""
    from orip import gcode as GC, stream_preview as SP
    text = CC.preview_gcode()
    W, H = 400, 300
    ink = {}
    for name, kw in (("plain", {}), ("clip", {"clip": True}), ("margin", {"clip": True, "clip_margin_mm": 1.0})):
        data, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(**dict(CC.PREVIEW_GCODE_ARGS, **kw)), dev)
        img, st = SP.preview(dev, data, W, H, W, H, invert_y=True)
        assert img.shape == (H, W, 3) and st["off_canvas_draws"] == 0 and st["eof_seen"] == 1 and st["steps_total"] == info["steps"]
        ink[name] = (img != 255).any(2)
    assert ink["plain"][:, 0].sum() >= 195                                           # 200 steps of border on the left
    rows = np.flatnonzero(ink["clip"][:, 0])
    assert 1 <= len(rows) <= 6 and set(rows.tolist()) <= set(range(H - 1 - 250 - 1, H - 1 - 250 + 2)) | set(range(H - 1 - 50 - 1, H - 1 - 50 + 2))      # the cuts at y = 50 and y = 250
    assert not ink["clip"][:, W - 1].any() and ink["clip"][:, 1:100].any()
    assert not ink["margin"][:, :4].any() and not ink["margin"][:, W - 4:].any() and ink["margin"][:, 4:100].any()
