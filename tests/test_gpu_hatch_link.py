"""--hatch-connect on the GPU: orip_gcode_hatch_link and orip_svg_hatch_link against the sequential double of tests/hatch_link_double.py -- off, pts,
member_off, member and all eight counts, by equality -- on every named drawing of tests/hatch_link_cases.py; the explicit and the resident form; the rings
converted on the device behind a real flatten, fit, hatch and conversion; the resident list and the sources afterwards; every argument check, with the
resident polylines left as they were; the consequences that need no double; and svg2stream's --hatch-connect end to end.  No comparison has a tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hatch_double as HD
import hatch_link_cases as LC
import hatch_link_double as LD
import merge_cases as MC
import occlude_double as OD

TOP = 1 << 30
CASES = LC.cases()
MAP = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=1.0, W=4000, H=4000, invert_y=0)
WANT = {}


def want(name):
    """the double's answer, computed once"""
    if name not in WANT:
        WANT[name] = LD.hatch_link(*LC.args(CASES[name]))
    return WANT[name]


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def equal(got, exp):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int64 and got[3].dtype == np.int32
    for k, (a, b) in enumerate(zip(got[:4], exp[:4])):
        assert a.shape == b.shape and np.array_equal(a, b), (k, a[:8], b[:8])
    assert got[4] == exp[4]


# ------------------------------------------------------------------ every drawing against the double
@pytest.mark.parametrize("name", sorted(CASES))
def test_case(dev, name):
    exp = want(name)
    got = dev.gcode_hatch_link(*LC.args(CASES[name]))
    equal(got, exp)
    f_off, f_pts = dev.gcode_steps_fetch(len(exp[0]) - 1, len(exp[1]))           # the result is the resident list
    assert np.array_equal(f_off, exp[0]) and np.array_equal(f_pts, exp[1])


@pytest.mark.parametrize("name", ["sixteen_shapes", "random_lines", "star_0", "star_1", "star_2", "many_starts", "ring_with_hole"])
def test_the_consequences_that_need_no_double(dev, name):
    LC.check_consequences(CASES[name], dev.gcode_hatch_link(*LC.args(CASES[name])))


@pytest.mark.parametrize("name", ["slit", "cross_hatch", "mixed_with_outlines", "sixteen_shapes", "coincident", "no_rings"])
def test_resident_form(dev, name):
    c = CASES[name]
    n = len(c["off"]) - 1
    none = (np.zeros(1, np.int64), np.zeros((0, 2), np.int32), np.zeros(0, np.int32))
    up = dev.gcode_hatch_link(c["off"], c["pts"], c["cls"], *none, c["reach"])  # without rings nothing links: the input becomes the resident list as it is
    assert np.array_equal(up[0], c["off"]) and np.array_equal(up[1], c["pts"]) and up[4]["links"] == 0 and up[3].tolist() == list(range(n))
    equal(dev.gcode_hatch_link(None, None, c["cls"], c["ring_off"], c["ring_pts"], c["ring_group"], c["reach"], n=n), want(name))


@pytest.mark.parametrize("shape,inset,strokes,clamp", [(LC.SQUARE, 27, 1, True), (LC.SLIT, 5, 2, True), (LC.SLIT, 5, 2, False)])
def test_svg_form_behind_flatten_fit_hatch_and_conversion(dev, shape, inset, strokes, clamp):
    t = HD.polys_table([[np.asarray(shape + shape[:1], np.float64)]])
    fg = np.array([0], np.int32)
    dev.svg_flatten(t, 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    st = dev.svg_hatch(fg, 1.0, 40, inset, HD.HORIZONTAL | HD.SERPENTINE)
    n_all = t.n_sub + st["segments"]
    p_off, p_mm = dev.svg_paths(n_all)
    groups = dev.svg_hatch_groups(st["segments"])
    if clamp:
        off, pts = dev.gcode_to_steps(None, None, MAP, n=n_all)
    else:
        off, pts, _ = dev.gcode_to_steps_clip(None, None, MAP, (0, 0, 3999, 3999), n=n_all)
    n = len(off) - 1
    src = dev.gcode_steps_source(n)
    cls = np.where(src < t.n_sub, -1, 2 * groups[np.maximum(src - t.n_sub, 0)]).astype(np.int32)
    r_off, r_pts = OD.rings_to_steps(p_off, p_mm, [0], MAP, clamp)
    exp = LD.hatch_link(off, pts, cls, r_off, r_pts, [0], 80)
    got = dev.svg_hatch_link(cls, [0], [0], MAP, clamp, 80, n=n)
    equal(got, exp)
    assert exp[4]["lines"] == st["segments"] and exp[4]["paths_out"] == 1 + strokes                   # the outline and the zigzags
    k = len(exp[0]) - 1
    f_off, f_pts = dev.gcode_steps_fetch(k, len(exp[1]))
    assert np.array_equal(f_off, exp[0]) and np.array_equal(f_pts, exp[1])
    assert dev.gcode_steps_source(k).tolist() == src[exp[3][exp[2][:-1]]].tolist()                    # the sources, gathered through every stroke's first member
    equal(dev.gcode_hatch_link(off, pts, cls, r_off, r_pts, [0], 80), exp)                           # and the explicit form with the same rings in steps


def test_nothing_to_link(dev):
    c = CASES["empty"]
    got = dev.gcode_hatch_link(*LC.args(c))
    equal(got, want("empty"))
    assert got[4] == dict.fromkeys(LD.STATS, 0)
    off, pts = dev.gcode_steps_fetch(0, 0)
    assert off.tolist() == [0] and len(pts) == 0


# ------------------------------------------------------------------ bad arguments
def raw(dev, off, pts, cls, n, ring_off, ring_pts, ring_group, m, reach, stats=True):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = np.full(8, -7, np.int64)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((off, np.int64), (pts, np.int32), (cls, np.int32), (ring_off, np.int64), (ring_pts, np.int32), (ring_group, np.int32))]
    rc = dev.L.orip_gcode_hatch_link(dev.h, p(keep[0]), p(keep[1]), p(keep[2]), int(n), p(keep[3]), p(keep[4]), p(keep[5]), int(m), int(reach), p(st) if stats else None)
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def raw_svg(dev, cls, n, ring_sub, ring_group, m, map_, flags, reach, stats=True):
    from orip import lib as _l
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = np.full(8, -7, np.int64)
    keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (cls, ring_sub, ring_group)]
    gm = None if map_ is None else C.byref(_l.GcodeMap(**{k: map_[k] for k, _ in _l.GcodeMap._fields_}))
    rc = dev.L.orip_svg_hatch_link(dev.h, p(keep[0]), int(n), p(keep[1]), p(keep[2]), int(m), gm, int(flags), int(reach), p(st) if stats else None)
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def mm_input():
    paths = [[(10, 10), (30, 10), (30, 30), (10, 30), (10, 10)], [(50, 50), (50, 50.2)], [(12, 14), (28, 14)], [(28, 18), (12, 18)]]
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return off, np.asarray([q for p in paths for q in p], np.float64)


def test_bad_arguments_leave_the_resident_paths(dev):
    dev.svg_flatten(HD.polys_table([[np.array([[1.0, 1.0], [9.0, 1.0], [5.0, 8.0]])]]), 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)      # one fitted path resident
    off_mm, mm = mm_input()
    off0, pts0 = dev.gcode_to_steps(off_mm, mm, MAP)
    n0, t0 = len(off0) - 1, len(pts0)
    src0 = dev.gcode_steps_source(n0)
    assert src0.tolist() == [0, 2, 3]
    o = np.array([0, 2, 5]); p = np.array([[1, 1], [2, 2], [2, 2], [3, 3], [9, 3]]); cl = np.array([0, 1])
    ro = np.array([0, 3, 4]); rp = np.array([[0, 0], [5, 0], [0, 5], [7, 7]]); rg = np.array([1, 1])
    bad = [("n < 0", (o, p, cl, -1, ro, rp, rg, 2, 8)), ("n > 2^26", (o, p, cl, (1 << 26) + 1, ro, rp, rg, 2, 8)), ("2^28 points", (np.array([0, 2, 1 << 28]), p, cl, 2, ro, rp, rg, 2, 8)),
           ("off[0] != 0", (np.array([1, 2, 5]), p, cl, 2, ro, rp, rg, 2, 8)), ("off decreases", (np.array([0, 3, 2]), p, cl, 2, ro, rp, rg, 2, 8)),
           ("a path of one point", (np.array([0, 4, 5]), p, cl, 2, ro, rp, rg, 2, 8)), ("x < 0", (o, np.array([[1, 1], [2, 2], [-1, 2], [3, 3], [9, 3]]), cl, 2, ro, rp, rg, 2, 8)),
           ("y > 2^30", (o, np.array([[1, 1], [2, 2], [2, 2], [3, TOP + 1], [9, 3]]), cl, 2, ro, rp, rg, 2, 8)),
           ("a point twice", (o, np.array([[1, 1], [2, 2], [2, 2], [3, 3], [3, 3]]), cl, 2, ro, rp, rg, 2, 8)),
           ("pts NULL", (o, None, cl, 2, ro, rp, rg, 2, 8)), ("off NULL", (None, p, cl, 2, ro, rp, rg, 2, 8)), ("cls NULL", (o, p, None, 2, ro, rp, rg, 2, 8)),
           ("cls < -1", (o, p, np.array([0, -2]), 2, ro, rp, rg, 2, 8)),
           ("m < 0", (o, p, cl, 2, ro, rp, rg, -1, 8)), ("m > 2^26", (o, p, cl, 2, ro, rp, rg, (1 << 26) + 1, 8)), ("2^28 ring points", (o, p, cl, 2, np.array([0, 3, 1 << 28]), rp, rg, 2, 8)),
           ("ring_off[0] != 0", (o, p, cl, 2, np.array([1, 3, 4]), rp, rg, 2, 8)), ("ring_off decreases", (o, p, cl, 2, np.array([0, 3, 2]), rp, rg, 2, 8)),
           ("a ring of no points", (o, p, cl, 2, np.array([0, 4, 4]), rp, rg, 2, 8)), ("ring x > 2^30", (o, p, cl, 2, ro, np.array([[0, 0], [TOP + 1, 0], [0, 5], [7, 7]]), rg, 2, 8)),
           ("ring y < -2^30", (o, p, cl, 2, ro, np.array([[0, 0], [5, 0], [0, -TOP - 1], [7, 7]]), rg, 2, 8)), ("ring_group decreases", (o, p, cl, 2, ro, rp, np.array([2, 1]), 2, 8)),
           ("ring_group < 0", (o, p, cl, 2, ro, rp, np.array([-1, 1]), 2, 8)), ("ring_group 2^30", (o, p, cl, 2, ro, rp, np.array([1, TOP]), 2, 8)),
           ("ring_off NULL", (o, p, cl, 2, None, rp, rg, 2, 8)), ("ring_pts NULL", (o, p, cl, 2, ro, None, rg, 2, 8)), ("ring_group NULL", (o, p, cl, 2, ro, rp, None, 2, 8)),
           ("reach 0", (o, p, cl, 2, ro, rp, rg, 2, 0)), ("reach < 0", (o, p, cl, 2, ro, rp, rg, 2, -5)), ("reach > 2^20", (o, p, cl, 2, ro, rp, rg, 2, (1 << 20) + 1)),
           ("not the resident count", (None, None, np.array([0] * (n0 + 1)), n0 + 1, ro, rp, rg, 2, 8)), ("not the resident count", (None, None, None, 0, ro, rp, rg, 2, 8))]
    for what, args in bad:
        rc, msg = raw(dev, *args)
        assert rc != 0 and "orip_gcode_hatch_link" in msg, what
    rc, msg = raw(dev, o, p, cl, 2, ro, rp, rg, 2, 8, stats=False)
    assert rc != 0 and "orip_gcode_hatch_link" in msg
    c0 = np.array([-1, 0, 0], np.int32); rs = np.array([0]); r1 = np.array([0])
    bad_svg = [("ring_sub < 0", (c0, n0, np.array([-1]), r1, 1, MAP, 0, 8)), ("ring_sub past the fitted paths", (c0, n0, np.array([1]), r1, 1, MAP, 0, 8)),
               ("unknown flags", (c0, n0, rs, r1, 1, MAP, 2, 8)), ("map NULL", (c0, n0, rs, r1, 1, None, 0, 8)), ("W 0", (c0, n0, rs, r1, 1, dict(MAP, W=0), 0, 8)),
               ("not the resident count", (np.zeros(n0 + 1, np.int32), n0 + 1, rs, r1, 1, MAP, 0, 8)), ("cls NULL", (None, n0, rs, r1, 1, MAP, 0, 8)),
               ("cls < -1", (np.full(n0, -2), n0, rs, r1, 1, MAP, 0, 8)), ("ring_sub NULL", (c0, n0, None, r1, 1, MAP, 0, 8)), ("ring_group NULL", (c0, n0, rs, None, 1, MAP, 0, 8)),
               ("ring_group decreases", (c0, n0, np.array([0, 0]), np.array([2, 1]), 2, MAP, 0, 8)), ("m < 0", (c0, n0, rs, r1, -1, MAP, 0, 8)),
               ("reach 0", (c0, n0, rs, r1, 1, MAP, 0, 0)), ("reach > 2^20", (c0, n0, rs, r1, 1, MAP, 0, (1 << 20) + 1))]
    for what, args in bad_svg:
        rc, msg = raw_svg(dev, *args)
        assert rc != 0 and "orip_svg_hatch_link" in msg, what
    rc, msg = raw_svg(dev, c0, n0, rs, r1, 1, MAP, 0, 8, stats=False)
    assert rc != 0 and "orip_svg_hatch_link" in msg
    off1, pts1 = dev.gcode_steps_fetch(n0, t0)                                   # the list and the context are as they were
    assert np.array_equal(off1, off0) and np.array_equal(pts1, pts0) and np.array_equal(dev.gcode_steps_source(n0), src0)
    rc, msg = raw_svg(dev, c0, n0, rs, r1, 1, MAP, 1, 8)                         # and arguments without a fault are taken, in both forms
    assert rc == 0, msg
    rc, msg = raw(dev, o, p, cl, 2, ro, rp, rg, 2, 8)
    assert rc == 0, msg
    from orip.device import OripError
    with pytest.raises(OripError):
        dev._ck(dev.L.orip_gcode_hatch_link_fetch(dev.h, None, None))            # a result and nowhere to put it


def test_a_ring_that_cannot_be_converted_leaves_no_list(dev):
    from orip.device import OripError
    dev.svg_flatten(HD.polys_table([[np.array([[1.0, 1.0], [9.0, 1.0], [5.0, 8.0]])]]), 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    off_mm, mm = mm_input()
    off0, _ = dev.gcode_to_steps(off_mm, mm, MAP)
    n0 = len(off0) - 1
    with pytest.raises(OripError, match="2\\^30"):
        dev.svg_hatch_link(np.full(n0, -1, np.int32), [0], [0], dict(MAP, steps_per_mm=1e12), False, 8, n=n0)      # found on the device: the drawing is that far off the sheet
    with pytest.raises(OripError):
        dev.gcode_steps_fetch(n0, 1)


# ------------------------------------------------------------------ the whole tool
def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def host_doubles(link=None):
    import clip_double as CD
    return dict(CD.svg_doubles(), hatch_link_fn=link)


def test_svg_tool_on_the_l_shape(dev):
    from orip import svg as SV
    link = LC.HatchLinkDouble()
    on = svg_options(LC.TOOL_ARGS + ["--hatch-connect"])
    exp, winfo = SV.build_stream_from_svg(LC.TOOL_SVG_L, on, **host_doubles(link))
    got, info = SV.build_stream_from_svg(LC.TOOL_SVG_L, on, dev)
    assert got == exp and info["hatch_link"] == winfo["hatch_link"] and info["paths"] == winfo["paths"]
    plain, pinfo = SV.build_stream_from_svg(LC.TOOL_SVG_L, svg_options(LC.TOOL_ARGS), dev)
    assert plain == SV.build_stream_from_svg(LC.TOOL_SVG_L, svg_options(LC.TOOL_ARGS), **host_doubles())[0] and "hatch_link" not in pinfo      # identical bytes without the option
    st = link.out[4]
    assert st["links"] > 0 and len(MC.strokes_of(got)) == st["paths_out"] == len(MC.strokes_of(plain)) - st["links"]      # pen-down events: exactly as many as the double says


@pytest.mark.parametrize("extra", [["--occlude", "--pen-colors", "#f00,#00f", "--dedup", "--merge-paths"], ["--clip", "--hatch-direction", "cross", "--allow-reverse"]])
def test_svg_tool_with_the_passes_around_it(dev, extra):
    from orip import svg as SV
    import dedup_double as DD
    import occlude_cases as OC
    args = svg_options(LC.TOOL_ARGS + ["--hatch-connect"] + extra)
    exp, winfo = SV.build_stream_from_svg(LC.TOOL_SVG, args, **dict(host_doubles(LC.HatchLinkDouble()), dedup_fn=DD.dedup_numpy, occlude_fn=OC.OccludeDouble()))
    got, info = SV.build_stream_from_svg(LC.TOOL_SVG, args, dev)
    assert got == exp and info["hatch_link"] == winfo["hatch_link"] and info.get("occlude") == winfo.get("occlude") and info.get("merge") == winfo.get("merge")
