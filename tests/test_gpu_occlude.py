"""--occlude on the GPU: orip_gcode_occlude and orip_svg_occlude against the sequential double of tests/occlude_double.py -- off, pts, origin and all ten
counts, by equality -- on every named drawing of tests/occlude_cases.py, the hand-worked answers and seeded random drawings; the resident form behind the
conversion, behind the clip, and behind a flatten, fit and hatch with the rings converted on the device; what the sources say afterwards; the uploaded
form with and without a resident list; every argument check, with the resident polylines left as they were; idempotence on rectilinear drawings; and
svg2stream.py --occlude against the host flow run through the doubles.  No comparison has a tolerance and no case is left out."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import occlude_cases as OC
import occlude_double as OD
import hatch_double as HD
import pens_double as PD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
TOP = 1 << 30
CASES = OC.cases()
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


def lists(off, pts):
    return [[tuple(q) for q in pts[a:b].tolist()] for a, b in zip(off[:-1], off[1:])]


# ------------------------------------------------------------------ every drawing against the double
def test_nothing_to_occlude(dev):
    a = OC.arrays(([], [], [OC.sq(0, 0, 5, 5)], [1]))
    got = dev.gcode_occlude(*a)
    equal(got, OD.occlude_numpy(*a))
    assert got[3] == dict.fromkeys(OD.STATS, 0)
    off, pts = dev.gcode_steps_fetch(0, 0)
    assert off.tolist() == [0] and len(pts) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_case(dev, name):
    a = OC.arrays(CASES[name])
    want = OD.occlude_numpy(*a)
    got = dev.gcode_occlude(*a)
    equal(got, want)
    f_off, f_pts = dev.gcode_steps_fetch(len(want[0]) - 1, len(want[1]))
    assert np.array_equal(f_off, want[0]) and np.array_equal(f_pts, want[1])


def test_what_the_named_cases_reach(dev):
    """the cases are there for the paths of the kernel they take: say so of the input, through the double"""
    assert OD.occlude_numpy(*OC.arrays(CASES["comb_of_70_teeth"]))[3]["pieces"] == 71            # more events on one segment than a wave has lanes
    assert len(CASES["polygon_of_200_edges"][2][0]) == 200                                       # more edges than one pass of the lanes
    st = OD.occlude_numpy(*OC.arrays(CASES["scatter"]))[3]
    assert st["segments"] > 512 and st["whole"] > 100 and st["cut"] > 20 and st["hidden"] > 0    # several blocks; the cull takes and refuses
    strokes, levels, rings, ring_levels = CASES["sliver_at_2_to_30"]
    shapes = OD._shapes(OC.offsets(rings).tolist(), rings[0], ring_levels)
    (a, b), (c, d) = OD.segment_pieces(strokes[0][0], strokes[0][1], shapes)
    assert b < c and float(b) == float(c) and max(max(p) for p in rings[0]) == TOP                # two distinct parameters that are one double


def test_hand_worked_answers(dev):
    for case, out, origin, counts in OC.HAND:
        got = dev.gcode_occlude(*OC.arrays(case))
        assert lists(got[0], got[1]) == out
        assert origin is None or got[2].tolist() == origin
        assert all(got[3][k] == v for k, v in counts.items())
    case, out = OC.HAND_TRIANGLE
    s, o = OC.shifted(case, OC.TRI_SHIFT), [[(x + OC.TRI_SHIFT, y) for x, y in p] for p in out]
    got = dev.gcode_occlude(*OC.arrays(s))
    assert lists(got[0], got[1]) == o
    got = dev.gcode_occlude(*OC.arrays(OC.reverse_stroke(s, 0)))
    assert lists(got[0], got[1]) == [p[::-1] for p in o[::-1]]


def test_random_oblique_drawings(dev):
    for seed in range(300):
        a = OC.arrays(OC.random_oblique(seed))
        equal(dev.gcode_occlude(*a), OD.occlude_numpy(*a))


def test_random_rectilinear_drawings_and_idempotence(dev):
    for seed in range(100):
        case = OC.random_rectilinear(seed)
        a = OC.arrays(case)
        want = OD.occlude_numpy(*a)
        got = dev.gcode_occlude(*a)
        equal(got, want)
        k = len(want[0]) - 1
        again = dev.gcode_occlude(None, None, a[2][want[2]], *a[3:], n=k)      # the resident result once more: nothing changes
        assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1]) and np.array_equal(again[2], np.arange(k))
        assert again[3]["whole"] == again[3]["segments"] and again[3]["draw_steps_in"] == again[3]["draw_steps_out"] == want[3]["draw_steps_out"]


def test_many_random_drawings_in_one_call(dev):
    """the random drawings side by side in one call, shifted apart and their levels kept apart: more than one block, boxes that meet and boxes that do not"""
    strokes, levels, rings = [], [], []
    for seed in range(200):
        s, lv, r, rl = OC.shifted(OC.random_oblique(seed), 3 + 18 * (seed % 15), 3 + 18 * (seed // 15))
        strokes += s; levels += [8 * seed + v for v in lv]; rings += [(8 * seed + v, q) for v, q in zip(rl, r)]
    a = OC.arrays((strokes, levels, [q for _, q in rings], [v for v, _ in rings]))
    equal(dev.gcode_occlude(*a), OD.occlude_numpy(*a))


# ------------------------------------------------------------------ the resident form
def mm_input():
    """a drawing in mm on a grid of one step per mm: a square, a path the conversion drops, a long stroke through the square, one that leaves the sheet"""
    paths = [OC.closed(OC.sq(10, 10, 30, 30)), [(50, 50), (50, 50.2)], [(0, 20), (60, 20), (60, 25), (0, 25)], [(-20, 15), (25, 15)]]
    off = OC.offsets(paths)
    return off, np.asarray([q for p in paths for q in p], np.float64)


RINGS = OC.arrays(([], [], [OC.sq(10, 10, 30, 30), OC.sq(-40, 12, 5, 18)], [1, 2]))[3:]


def test_resident_form_behind_the_conversion(dev):
    off_mm, mm = mm_input()
    off, pts = dev.gcode_to_steps(off_mm, mm, MAP)
    n = len(off) - 1
    src = dev.gcode_steps_source(n)
    assert src.tolist() == [0, 2, 3]
    level = np.array([1, 0, 0], np.int32)
    want = OD.occlude_numpy(off, pts, level, *RINGS)
    got = dev.gcode_occlude(None, None, level, *RINGS, n=n)
    equal(got, want)
    assert want[3]["cut"] >= 3 and want[3]["whole"] >= 4
    k = len(want[0]) - 1
    f_off, f_pts = dev.gcode_steps_fetch(k, len(want[1]))
    assert np.array_equal(f_off, want[0]) and np.array_equal(f_pts, want[1])
    assert dev.gcode_steps_source(k).tolist() == src[want[2]].tolist()          # the input path of every stroke, gathered through origin
    m = dev.gcode_merge(None, None, None, 1, True, n=k)                         # the pieces are what the passes behind take
    assert m[5]["paths_out"] <= k
    from orip.device import OripError
    with pytest.raises(OripError):
        dev.gcode_steps_source(len(m[0]) - 1)


def test_resident_form_behind_the_clip(dev):
    off_mm, mm = mm_input()
    off, pts, _ = dev.gcode_to_steps_clip(off_mm, mm, MAP, (0, 0, 55, 3999))
    n = len(off) - 1
    src = dev.gcode_steps_source(n)
    level = (src == 0).astype(np.int32)
    want = OD.occlude_numpy(off, pts, level, *RINGS)
    equal(dev.gcode_occlude(None, None, level, *RINGS, n=n), want)
    assert dev.gcode_steps_source(len(want[0]) - 1).tolist() == src[want[2]].tolist()
    # the ring that lies half off the sheet still hides the stroke that was cut at the sheet's edge
    assert [(0, 15), (5, 15)] not in lists(want[0], want[1]) and any(s[0] == (5, 15) for s in lists(want[0], want[1]))


@pytest.mark.parametrize("clamp", [True, False])
def test_svg_occlude_behind_flatten_fit_and_hatch(dev, clamp):
    """two filled polygons, the second half off the sheet, hatched; the strokes are converted and the rings are the fitted paths themselves"""
    polys = [[np.array([[100.3, 100.2], [900.4, 100.7], [900.1, 700.6], [100.9, 700.5]])], [np.array([[-300.2, 300.4], [500.6, 350.5], [200.5, 900.3]])]]
    t = HD.polys_table(polys)
    fg = np.array([0, 1], np.int32)
    dev.svg_flatten(t, 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    st = dev.svg_hatch(fg, 2.0, 40, 3, HD.HORIZONTAL)
    n_all = t.n_sub + st["segments"]
    p_off, p_mm = dev.svg_paths(n_all)
    groups = dev.svg_hatch_groups(st["segments"])
    m = dict(MAP, steps_per_mm=2.0, W=1600, H=1600, invert_y=1)
    if clamp:
        off, pts = dev.gcode_to_steps(None, None, m, n=n_all)
    else:
        off, pts, _ = dev.gcode_to_steps_clip(None, None, m, (0, 0, 1599, 1599), n=n_all)
    n = len(off) - 1
    src = dev.gcode_steps_source(n)
    level = np.where(src < t.n_sub, fg[np.minimum(src, t.n_sub - 1)], groups[np.maximum(src - t.n_sub, 0)]).astype(np.int32)
    ring_sub, ring_level = np.array([0, 1], np.int32), fg
    r_off, r_pts = OD.rings_to_steps(p_off, p_mm, ring_sub.tolist(), m, clamp)
    want = OD.occlude_numpy(off, pts, level, r_off, r_pts, ring_level)
    got = dev.svg_occlude(level, ring_sub, ring_level, m, clamp, n=n)
    equal(got, want)
    assert want[3]["cut"] >= 20 and want[3]["whole"] >= 38                     # the outline of the lower polygon and half of its hatch lines run under the upper one
    assert dev.gcode_steps_source(len(want[0]) - 1).tolist() == src[want[2]].tolist()
    assert (r_pts.min() < 0) == (not clamp)


def drop_the_list(dev):
    rc = dev.L.orip_gcode_to_steps(dev.h, None, None, 0, None, None, None)     # the conversion drops the list before it looks at its arguments
    assert rc != 0
    with pytest.raises(Exception):
        dev.gcode_steps_fetch(0, 0)


def test_uploaded_form_and_the_sources(dev):
    from orip.device import OripError
    a = OC.arrays(CASES["levels_decide"])                                      # three strokes
    want = OD.occlude_numpy(*a)
    drop_the_list(dev)
    equal(dev.gcode_occlude(*a), want)                                         # no list resident: the strokes have no sources
    with pytest.raises(OripError):
        dev.gcode_steps_source(len(want[0]) - 1)
    off_mm, mm = mm_input()
    dev.gcode_to_steps(off_mm, mm, MAP)                                        # three strokes resident, as many as the case has: taken for the polylines a fetch gave out
    src = dev.gcode_steps_source(3)
    equal(dev.gcode_occlude(*a), want)
    assert dev.gcode_steps_source(len(want[0]) - 1).tolist() == src[want[2]].tolist()
    dev.gcode_to_steps(off_mm, mm, MAP)
    b = OC.arrays(CASES["hand_1"])                                             # another count: the sources do not name these
    equal(dev.gcode_occlude(*b), OD.occlude_numpy(*b))
    with pytest.raises(OripError):
        dev.gcode_steps_source(3)
    dev.gcode_to_steps(off_mm, mm, MAP)
    assert dev.gcode_steps_source(3).tolist() == [0, 2, 3]                     # and the next conversion names its sources again


# ------------------------------------------------------------------ bad arguments
def raw(dev, off, pts, level, n, ring_off, ring_pts, ring_level, m, stats=True):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = np.full(10, -7, np.int64)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((off, np.int64), (pts, np.int32), (level, np.int32), (ring_off, np.int64), (ring_pts, np.int32), (ring_level, np.int32))]
    rc = dev.L.orip_gcode_occlude(dev.h, p(keep[0]), p(keep[1]), p(keep[2]), int(n), p(keep[3]), p(keep[4]), p(keep[5]), int(m), p(st) if stats else None)
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def raw_svg(dev, level, n, ring_sub, ring_level, m, map_, flags, stats=True):
    from orip import lib as _l
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = np.full(10, -7, np.int64)
    keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (level, ring_sub, ring_level)]
    gm = None if map_ is None else C.byref(_l.GcodeMap(**{k: map_[k] for k, _ in _l.GcodeMap._fields_}))
    rc = dev.L.orip_svg_occlude(dev.h, p(keep[0]), int(n), p(keep[1]), p(keep[2]), int(m), gm, int(flags), p(st) if stats else None)
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def test_bad_arguments_leave_the_resident_paths(dev):
    dev.svg_flatten(HD.polys_table([[np.array([[1.0, 1.0], [9.0, 1.0], [5.0, 8.0]])]]), 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)      # one fitted path resident
    off_mm, mm = mm_input()
    off0, pts0 = dev.gcode_to_steps(off_mm, mm, MAP)
    n0, t0 = len(off0) - 1, len(pts0)
    src0 = dev.gcode_steps_source(n0)
    o = np.array([0, 2, 5]); p = np.array([[1, 1], [2, 2], [2, 2], [3, 3], [9, 3]]); lv = np.array([0, 1])
    ro = np.array([0, 3, 4]); rp = np.array([[0, 0], [5, 0], [0, 5], [7, 7]]); rl = np.array([1, 1])
    bad = [("n < 0", (o, p, lv, -1, ro, rp, rl, 2)), ("n > 2^26", (o, p, lv, (1 << 26) + 1, ro, rp, rl, 2)), ("2^28 points", (np.array([0, 2, 1 << 28]), p, lv, 2, ro, rp, rl, 2)),
           ("off[0] != 0", (np.array([1, 2, 5]), p, lv, 2, ro, rp, rl, 2)), ("off decreases", (np.array([0, 3, 2]), p, lv, 2, ro, rp, rl, 2)),
           ("a path of one point", (np.array([0, 4, 5]), p, lv, 2, ro, rp, rl, 2)), ("x < 0", (o, np.array([[1, 1], [2, 2], [-1, 2], [3, 3], [9, 3]]), lv, 2, ro, rp, rl, 2)),
           ("y > 2^30", (o, np.array([[1, 1], [2, 2], [2, 2], [3, TOP + 1], [9, 3]]), lv, 2, ro, rp, rl, 2)),
           ("a point twice", (o, np.array([[1, 1], [2, 2], [2, 2], [3, 3], [3, 3]]), lv, 2, ro, rp, rl, 2)),
           ("pts NULL", (o, None, lv, 2, ro, rp, rl, 2)), ("off NULL", (None, p, lv, 2, ro, rp, rl, 2)), ("level NULL", (o, p, None, 2, ro, rp, rl, 2)),
           ("level < 0", (o, p, np.array([0, -1]), 2, ro, rp, rl, 2)), ("level 2^30", (o, p, np.array([0, TOP]), 2, ro, rp, rl, 2)),
           ("m < 0", (o, p, lv, 2, ro, rp, rl, -1)), ("m > 2^26", (o, p, lv, 2, ro, rp, rl, (1 << 26) + 1)), ("2^28 ring points", (o, p, lv, 2, np.array([0, 3, 1 << 28]), rp, rl, 2)),
           ("ring_off[0] != 0", (o, p, lv, 2, np.array([1, 3, 4]), rp, rl, 2)), ("ring_off decreases", (o, p, lv, 2, np.array([0, 3, 2]), rp, rl, 2)),
           ("a ring of no points", (o, p, lv, 2, np.array([0, 4, 4]), rp, rl, 2)), ("ring x > 2^30", (o, p, lv, 2, ro, np.array([[0, 0], [TOP + 1, 0], [0, 5], [7, 7]]), rl, 2)),
           ("ring y < -2^30", (o, p, lv, 2, ro, np.array([[0, 0], [5, 0], [0, -TOP - 1], [7, 7]]), rl, 2)), ("ring_level decreases", (o, p, lv, 2, ro, rp, np.array([2, 1]), 2)),
           ("ring_level < 0", (o, p, lv, 2, ro, rp, np.array([-1, 1]), 2)), ("ring_level 2^30", (o, p, lv, 2, ro, rp, np.array([1, TOP]), 2)),
           ("ring_off NULL", (o, p, lv, 2, None, rp, rl, 2)), ("ring_pts NULL", (o, p, lv, 2, ro, None, rl, 2)), ("ring_level NULL", (o, p, lv, 2, ro, rp, None, 2)),
           ("not the resident count", (None, None, np.array([0] * (n0 + 1)), n0 + 1, ro, rp, rl, 2)), ("not the resident count", (None, None, None, 0, ro, rp, rl, 2))]
    for what, args in bad:
        rc, msg = raw(dev, *args)
        assert rc != 0 and "orip_gcode_occlude" in msg, what
    rc, msg = raw(dev, o, p, lv, 2, ro, rp, rl, 2, stats=False)
    assert rc != 0 and "orip_gcode_occlude" in msg
    l0 = np.zeros(n0, np.int32); rs = np.array([0]); r1 = np.array([1])
    bad_svg = [("ring_sub < 0", (l0, n0, np.array([-1]), r1, 1, MAP, 0)), ("ring_sub past the fitted paths", (l0, n0, np.array([1]), r1, 1, MAP, 0)),
               ("unknown flags", (l0, n0, rs, r1, 1, MAP, 2)), ("map NULL", (l0, n0, rs, r1, 1, None, 0)), ("W 0", (l0, n0, rs, r1, 1, dict(MAP, W=0), 0)),
               ("not the resident count", (np.zeros(n0 + 1, np.int32), n0 + 1, rs, r1, 1, MAP, 0)), ("level NULL", (None, n0, rs, r1, 1, MAP, 0)),
               ("level out of range", (np.full(n0, TOP), n0, rs, r1, 1, MAP, 0)), ("ring_sub NULL", (l0, n0, None, r1, 1, MAP, 0)), ("ring_level NULL", (l0, n0, rs, None, 1, MAP, 0)),
               ("ring_level decreases", (l0, n0, np.array([0, 0]), np.array([2, 1]), 2, MAP, 0)), ("m < 0", (l0, n0, rs, r1, -1, MAP, 0))]
    for what, args in bad_svg:
        rc, msg = raw_svg(dev, *args)
        assert rc != 0 and "orip_svg_occlude" in msg, what
    rc, msg = raw_svg(dev, l0, n0, rs, r1, 1, MAP, 0, stats=False)
    assert rc != 0 and "orip_svg_occlude" in msg
    off1, pts1 = dev.gcode_steps_fetch(n0, t0)
    assert np.array_equal(off1, off0) and np.array_equal(pts1, pts0) and np.array_equal(dev.gcode_steps_source(n0), src0)
    rc, msg = raw_svg(dev, l0, n0, rs, r1, 1, MAP, 1)                          # and arguments without a fault are taken, in both forms
    assert rc == 0, msg
    rc, msg = raw(dev, o, p, lv, 2, ro, rp, rl, 2)
    assert rc == 0, msg
    from orip.device import OripError
    with pytest.raises(OripError):
        dev._ck(dev.L.orip_gcode_occlude_fetch(dev.h, None))                  # a result and nowhere to put it


def test_a_ring_that_cannot_be_converted_leaves_no_list(dev):
    from orip.device import OripError
    dev.svg_flatten(HD.polys_table([[np.array([[1.0, 1.0], [9.0, 1.0], [5.0, 8.0]])]]), 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    off_mm, mm = mm_input()
    off0, _ = dev.gcode_to_steps(off_mm, mm, MAP)
    n0 = len(off0) - 1
    with pytest.raises(OripError, match="2\\^30"):
        dev.svg_occlude(np.zeros(n0, np.int32), [0], [1], dict(MAP, steps_per_mm=1e12), False, n=n0)      # found on the device: the drawing is that far off the sheet
    with pytest.raises(OripError):
        dev.gcode_steps_fetch(n0, 1)


# ------------------------------------------------------------------ the whole tool
def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def host_doubles():
    import clip_double as CD
    import dedup_double as DD
    return dict(CD.svg_doubles(), dedup_fn=DD.dedup_numpy, occlude_fn=OC.OccludeDouble())


FULL = OC.TOOL_ARGS + ["--hatch-spacing-mm", "5", "--pen-colors", "#f00,#00f", "--dedup", "--merge-paths"]


@pytest.mark.parametrize("svg,args", [(OC.TOOL_SVG, OC.TOOL_ARGS), (OC.TOOL_SVG, FULL), (OC.TOOL_SVG, OC.TOOL_ARGS + ["--hatch-spacing-mm", "5", "--clip", "--simplify-mm", "0"]),
                                      (OC.TOOL_SVG_OFF_SHEET, OC.TOOL_ARGS + ["--clip"]), (OC.TOOL_SVG_OFF_SHEET, OC.TOOL_ARGS)])
def test_svg_tool_in_process(dev, svg, args):
    from orip import svg as SV
    dbl = host_doubles()
    if "--simplify-mm" in args:
        dbl["simplify_fn"] = __import__("simplify_double").simplify_numpy
    want, winfo = SV.build_stream_from_svg(svg, svg_options(args), **dbl)
    got, info = SV.build_stream_from_svg(svg, svg_options(args), dev)
    assert got == want and info["occlude"] == winfo["occlude"] and info["paths"] == winfo["paths"] and info.get("dedup") == winfo.get("dedup")
    assert info.get("merge") == winfo.get("merge") and info["occlude"]["cut"] > 0


def test_svg_tool_as_a_process(dev, tmp_path):
    from orip import svg as SV
    want, winfo = SV.build_stream_from_svg(OC.TOOL_SVG, svg_options(FULL), want_paths=True, **host_doubles())
    src = tmp_path / "drawing.svg"
    src.write_bytes(OC.TOOL_SVG)
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "svg2stream.py"), str(src), "--preview-render-width", "320", "--preview-render-height", "240"] + FULL,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = winfo["occlude"]
    line = (f"[svg] occlude: {d['segments']} segments: {d['whole']} whole, {d['cut']} cut, {d['hidden']} hidden -> {d['paths_out']} strokes, "
            f"pen-down steps {d['draw_steps_in']} -> {d['draw_steps_out']}")
    assert (tmp_path / "drawing_stream.bin").read_bytes() == want and line in r.stdout and (tmp_path / "drawing_stream_preview.png").exists()
    assert (tmp_path / "drawing.gcode").read_text() == SV.gcode_text(*winfo["fitted_paths"], pens=winfo["path_pens"])      # the G-code file does not know of the pass
