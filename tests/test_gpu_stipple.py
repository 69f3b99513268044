"""--stipple-mm on the GPU: orip_gcode_stipple and orip_svg_stipple against the sequential double of tests/stipple_double.py -- xy, group and all seven
counts, by equality -- on every named drawing of tests/stipple_cases.py; the svg form behind a real flatten, fit and conversion, clamped and not, with the
resident step polylines and their sources bit for bit what they were; every argument check, with the context still usable; the consequences that need no
double; and svg2stream's --stipple-mm end to end.  No comparison has a tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hatch_double as HD
import hatch_link_cases as LC
import occlude_double as OD
import stipple_cases as SC
import stipple_double as SD

TOP = 1 << 30
CASES = SC.cases()
MAP = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=1.0, W=1000, H=4000, invert_y=0)
WANT = {}


def want(name):
    """the double's answer, computed once"""
    if name not in WANT:
        WANT[name] = SD.stipple(*SC.args(CASES[name]))
    return WANT[name]


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def equal(got, exp):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[0].shape == exp[0].shape and got[1].shape == exp[1].shape
    assert got[2] == exp[2], (got[2], exp[2])
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (got[0][:8], exp[0][:8])


# ------------------------------------------------------------------ every drawing against the double
@pytest.mark.parametrize("name", sorted(CASES))
def test_case(dev, name):
    equal(dev.gcode_stipple(*SC.args(CASES[name])), want(name))


def test_the_square_has_529_dots(dev):
    xy, grp, st = dev.gcode_stipple(*SC.args(CASES["square"]))
    assert st["dots"] == 529 and xy.tolist() == [[x, y] for y in range(160, 1041, 40) for x in range(160, 1041, 40)] and not grp.any()


@pytest.mark.parametrize("name", ["gon_100", "negative_rows", "overlap_3_occlude", "comb_40_teeth", "many_squares"])
def test_the_consequences_that_need_no_double(dev, name):
    c = CASES[name]
    xy, grp, st = dev.gcode_stipple(*SC.args(c))
    (p, q, s), (x0, y0, x1, y1) = c["lattice"], c["rect"]
    x, y = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    assert st["candidates"] == st["near"] + st["outside"] + st["hidden"] + st["dots"] and st["dots"] == len(xy) == len(grp)
    assert not (y % q).any() and not ((x - np.where((y // q) & 1, s, 0)) % p).any() and (x >= x0).all() and (x <= x1).all() and (y >= y0).all() and (y <= y1).all()
    moved, v = SC.shifted(c, -3, 8)                                               # a lattice vector: the dots move with the drawing
    xy2, grp2, st2 = dev.gcode_stipple(*SC.args(moved))
    assert np.array_equal(xy2, xy + v.astype(np.int32)) and np.array_equal(grp2, grp) and st2 == st
    seen = {tuple(r) for r in np.column_stack([xy, grp]).tolist()}
    for inset in (c["inset"] + 1, c["inset"] + 40):                               # raising the inset never adds a dot
        xy3, grp3, st3 = dev.gcode_stipple(*SC.args(dict(c, inset=inset)))
        now = {tuple(r) for r in np.column_stack([xy3, grp3]).tolist()}
        assert now <= seen and st3["candidates"] == st["candidates"]
        seen = now


def test_the_top_shape_loses_nothing_under_the_occlude_flag(dev):
    plain, occ = dev.gcode_stipple(*SC.args(CASES["overlap_3"])), dev.gcode_stipple(*SC.args(CASES["overlap_3_occlude"]))
    top = int(CASES["overlap_3"]["ring_group"][-1])
    assert np.array_equal(plain[0][plain[1] == top], occ[0][occ[1] == top]) and occ[2]["hidden"] == plain[2]["dots"] - occ[2]["dots"] > 0 and plain[2]["hidden"] == 0


# ------------------------------------------------------------------ the svg form
@pytest.mark.parametrize("clamp", [True, False])
def test_svg_form_behind_flatten_fit_and_conversion(dev, clamp):
    shapes = [LC.SLIT, [(x + 400, y + 1500) for x, y in LC.SQUARE], LC.ngon(500, 3200, 450, 30)]      # the second leaves the sheet of 1000 x 4000 on the right
    t = HD.polys_table([[np.asarray(s + s[:1], np.float64)] for s in shapes])
    dev.svg_flatten(t, 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    p_off, p_mm = dev.svg_paths(t.n_sub)
    if clamp:
        off, pts = dev.gcode_to_steps(None, None, MAP, n=t.n_sub)
    else:
        off, pts, _ = dev.gcode_to_steps_clip(None, None, MAP, (0, 0, 999, 3999), n=t.n_sub)
    n = len(off) - 1
    src = dev.gcode_steps_source(n)
    ring_sub, ring_group = [0, 1, 2], [0, 4, 4]
    r_off, r_pts = OD.rings_to_steps(p_off, p_mm, ring_sub, MAP, clamp)
    assert (r_pts[:, 0].max() > 999) == (not clamp)
    for lattice, inset, flags in (((40, 35, 20), 27, SD.SERPENTINE), ((40, 40, 0), 0, SD.OCCLUDE)):
        exp = SD.stipple(r_off, r_pts, ring_group, lattice, inset, (0, 0, 999, 3999), flags)
        equal(dev.svg_stipple(ring_sub, ring_group, MAP, clamp, lattice, inset, (0, 0, 999, 3999), flags), exp)
        assert exp[2]["dots"] > 300 and (exp[2]["outside"] > 0) == (not clamp)
        equal(dev.gcode_stipple(r_off, r_pts, ring_group, lattice, inset, (0, 0, 999, 3999), flags), exp)      # and the explicit form with the same rings in steps
    f_off, f_pts = dev.gcode_steps_fetch(n, len(pts))                             # the pass writes neither the resident step polylines nor their sources
    assert np.array_equal(f_off, off) and np.array_equal(f_pts, pts) and np.array_equal(dev.gcode_steps_source(n), src)
    q_off, q_mm = dev.svg_paths(t.n_sub)
    assert np.array_equal(q_off, p_off) and np.array_equal(q_mm, p_mm)


# ------------------------------------------------------------------ bad arguments
def raw(dev, ring_off, ring_pts, ring_group, m, pitch, row, shift, inset, rect, flags, stats=True):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = np.full(7, -7, np.int64)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((ring_off, np.int64), (ring_pts, np.int32), (ring_group, np.int32), (rect, np.int32))]
    rc = dev.L.orip_gcode_stipple(dev.h, p(keep[0]), p(keep[1]), p(keep[2]), int(m), int(pitch), int(row), int(shift), int(inset), p(keep[3]), int(flags), p(st) if stats else None)
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def raw_svg(dev, ring_sub, ring_group, m, map_, pitch, row, shift, inset, rect, flags, stats=True):
    from orip import lib as _l
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = np.full(7, -7, np.int64)
    keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (ring_sub, ring_group, rect)]
    gm = None if map_ is None else C.byref(_l.GcodeMap(**{k: map_[k] for k, _ in _l.GcodeMap._fields_}))
    rc = dev.L.orip_svg_stipple(dev.h, p(keep[0]), p(keep[1]), int(m), gm, int(pitch), int(row), int(shift), int(inset), p(keep[2]), int(flags), p(st) if stats else None)
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def test_bad_arguments_leave_everything_as_it_was(dev):
    from orip.device import OripError
    dev.svg_flatten(HD.polys_table([[np.array([[100.0, 100.0], [900.0, 100.0], [500.0, 800.0]])]]), 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)      # one fitted path resident
    off0, pts0 = dev.gcode_to_steps(None, None, MAP, n=1)
    src0 = dev.gcode_steps_source(1)
    first = dev.gcode_stipple(*SC.args(CASES["l_shape"]))                         # a dot list that the failed calls must leave
    ro = np.array([0, 3, 4]); rp = np.array([[0, 0], [500, 0], [0, 500], [7, 7]]); rg = np.array([1, 1]); rc4 = np.array([0, 0, 999, 999])
    good = (ro, rp, rg, 2, 40, 35, 20, 27, rc4, 3)
    bad = [("m < 0", {3: -1}), ("m > 2^26", {3: (1 << 26) + 1}), ("2^28 ring points", {0: np.array([0, 3, 1 << 28])}), ("ring_off[0] != 0", {0: np.array([1, 3, 4])}),
           ("ring_off decreases", {0: np.array([0, 3, 2])}), ("a ring of no points", {0: np.array([0, 4, 4])}), ("ring x > 2^30", {1: np.array([[0, 0], [TOP + 1, 0], [0, 5], [7, 7]])}),
           ("ring y < -2^30", {1: np.array([[0, 0], [5, 0], [0, -TOP - 1], [7, 7]])}), ("ring_group decreases", {2: np.array([2, 1])}), ("ring_group < 0", {2: np.array([-1, 1])}),
           ("ring_group 2^30", {2: np.array([1, TOP])}), ("ring_off NULL", {0: None}), ("ring_pts NULL", {1: None}), ("ring_group NULL", {2: None}),
           ("pitch 1", {4: 1}), ("pitch 0", {4: 0}), ("pitch > 2^20", {4: (1 << 20) + 1, 6: 0}), ("row 0", {5: 0}), ("row < 0", {5: -3}), ("row > 2^20", {5: (1 << 20) + 1}),
           ("shift < 0", {6: -1}), ("shift == pitch", {6: 40}), ("inset < 0", {7: -1}), ("inset > 2^20", {7: (1 << 20) + 1}),
           ("x1 < x0", {8: np.array([10, 0, 9, 999])}), ("y1 < y0", {8: np.array([0, 10, 999, 9])}), ("rect beyond 2^30", {8: np.array([0, 0, TOP + 1, 999])}),
           ("rect below -2^30", {8: np.array([0, -TOP - 1, 999, 999])}), ("rect NULL", {8: None}), ("unknown flags", {9: 8}), ("the clamp flag without a map", {9: 4})]
    for what, change in bad:
        args = list(good)
        for k, v in change.items():
            args[k] = v
        rc, msg = raw(dev, *args)
        assert rc != 0 and "orip_gcode_stipple" in msg, what
    rc, msg = raw(dev, *good, stats=False)
    assert rc != 0 and "orip_gcode_stipple" in msg
    rs = np.array([0]); r1 = np.array([0])
    good_svg = (rs, r1, 1, MAP, 40, 35, 20, 27, rc4, 7)
    bad_svg = [("ring_sub < 0", {0: np.array([-1])}), ("ring_sub past the fitted paths", {0: np.array([1])}), ("unknown flags", {9: 8}), ("map NULL", {3: None}),
               ("W 0", {3: dict(MAP, W=0)}), ("H > 2^30", {3: dict(MAP, H=TOP + 1)}), ("ring_sub NULL", {0: None}), ("ring_group NULL", {1: None}),
               ("ring_group decreases", {0: np.array([0, 0]), 1: np.array([2, 1]), 2: 2}), ("m < 0", {2: -1}), ("pitch 1", {4: 1}), ("shift == pitch", {6: 40}),
               ("inset > 2^20", {7: (1 << 20) + 1}), ("x1 < x0", {8: np.array([10, 0, 9, 999])}), ("rect NULL", {8: None})]
    for what, change in bad_svg:
        args = list(good_svg)
        for k, v in change.items():
            args[k] = v
        rc, msg = raw_svg(dev, *args)
        assert rc != 0 and "orip_svg_stipple" in msg, what
    rc, msg = raw_svg(dev, *good_svg, stats=False)
    assert rc != 0 and "orip_svg_stipple" in msg
    xy = np.zeros((first[2]["dots"], 2), np.int32); grp = np.zeros(first[2]["dots"], np.int32)      # the dot list, the polylines and the context are as they were
    dev._ck(dev.L.orip_gcode_stipple_fetch(dev.h, xy.ctypes.data_as(C.c_void_p), grp.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(xy, first[0]) and np.array_equal(grp, first[1])
    with pytest.raises(OripError):
        dev._ck(dev.L.orip_gcode_stipple_fetch(dev.h, None, None))                # a result and nowhere to put it
    off1, pts1 = dev.gcode_steps_fetch(1, len(pts0))
    assert np.array_equal(off1, off0) and np.array_equal(pts1, pts0) and np.array_equal(dev.gcode_steps_source(1), src0)
    rc, msg = raw(dev, *good)                                                     # and arguments without a fault are taken, in both forms
    assert rc == 0, msg
    rc, msg = raw_svg(dev, *good_svg)
    assert rc == 0, msg
    rc, msg = raw(dev, None, None, None, 0, 40, 35, 20, 27, rc4, 3)               # m == 0: zeros, and the list of no dots
    assert rc == 0, msg
    dev._ck(dev.L.orip_gcode_stipple_fetch(dev.h, None, None))


def test_errors_found_on_the_device_leave_no_dot_list(dev):
    from orip.device import OripError
    dev.svg_flatten(HD.polys_table([[np.array([[1.0, 1.0], [9.0, 1.0], [5.0, 8.0]])]]), 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    dev.gcode_stipple(*SC.args(CASES["square"]))
    with pytest.raises(OripError, match="2\\^30"):
        dev.svg_stipple([0], [0], dict(MAP, steps_per_mm=1e12), False, (40, 40, 0), 27, (0, 0, 999, 999), 0)      # found on the device: the drawing is that far off the sheet
    with pytest.raises(OripError, match="no result"):
        dev._ck(dev.L.orip_gcode_stipple_fetch(dev.h, None, None))
    dev.gcode_stipple(*SC.args(CASES["square"]))
    with pytest.raises(OripError, match="2\\^28"):                                # 2^29 rows: refused behind the count, before any lattice point is looked at
        dev.gcode_stipple([0, 4], SC.rect_ring(0, 0, 1 << 29, 1 << 29), [0], (2, 1, 0), 0, (0, 0, TOP, TOP), 0)
    with pytest.raises(OripError, match="no result"):
        dev._ck(dev.L.orip_gcode_stipple_fetch(dev.h, None, None))
    equal(dev.gcode_stipple(*SC.args(CASES["square"])), want("square"))           # and the context is still usable


# ------------------------------------------------------------------ the whole tool
def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def host_doubles(stipple):
    import clip_double as CD
    import dedup_double as DD
    import occlude_cases as OC
    import seam_double as SM
    import simplify_double as SP
    return dict(CD.svg_doubles(), dedup_fn=DD.dedup_numpy, occlude_fn=OC.OccludeDouble(), seam_fn=SM.seams, simplify_fn=SP.simplify_numpy, stipple_fn=stipple)


STIPPLE = ["--stipple-mm", "4", "--stipple-inset-mm", "1.5"]


@pytest.mark.parametrize("extra", [[], ["--no-reorder", "--stipple-pattern", "square"], ["--pen-colors", "#00f,#f00,#000", "--occlude", "--clip", "--allow-reverse"],
                                   ["--hatch-spacing-mm", "4", "--dedup", "--merge-paths", "--simplify-mm", "0.1"]])
def test_svg_tool_against_the_doubles(dev, extra):
    from orip import svg as SV
    from test_stipple_host import taps_of
    Z = SC.StippleDouble()
    on = svg_options(SC.TOOL_ARGS + STIPPLE + extra)
    exp, winfo = SV.build_stream_from_svg(SC.TOOL_SVG, on, **host_doubles(Z))
    got, info = SV.build_stream_from_svg(SC.TOOL_SVG, on, dev)
    assert got == exp and info["stipple"] == winfo["stipple"] and info["taps"] == winfo["taps"] and info["paths"] == winfo["paths"]
    assert len(taps_of(got)) == info["stipple"]["dots"] > 100
    off = svg_options(SC.TOOL_ARGS + [a for a in extra if a not in ("--stipple-pattern", "square")])      # without the option: no pass, no tap
    plain, pinfo = SV.build_stream_from_svg(SC.TOOL_SVG, off, dev)
    assert "stipple" not in pinfo and not taps_of(plain) and plain == SV.build_stream_from_svg(SC.TOOL_SVG, off, **host_doubles(None))[0]


def test_main_stream_with_improve_order_and_loop_start(dev, tmp_path, capsys):
    from orip import svg as SV
    from test_stipple_host import taps_of
    (tmp_path / "in.svg").write_bytes(SC.TOOL_SVG)
    args = SC.TOOL_ARGS + STIPPLE + ["--improve-order", "--loop-start", "--allow-reverse", "--occlude"]
    SV.main_stream([str(tmp_path / "in.svg"), "--no-preview"] + args, device=dev)  # the seam pass is sent every dot as the open stroke P, P and takes it
    data = (tmp_path / "in_stream.bin").read_bytes()
    out = capsys.readouterr().out
    _, info = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(args), dev)
    d = info["stipple"]
    assert len(taps_of(data)) == d["dots"] == info["taps"] > 100 and d["hidden"] > 0 and info["seam"]["closed"] >= 1
    assert f"[svg] stipple: {d['dots']} dots in 2 shapes (pitch 40, rows 35; {d['near']} near the outline, 0 off the sheet, {d['hidden']} hidden)" in out
    assert (tmp_path / "in.gcode").read_text().count("M3") == 3                   # the G-code holds the three outlines and no dot
    seam, st = dev.gcode_seam(np.array([0, 2, 4]), np.array([[5, 5], [5, 5], [90, 5], [90, 5]]), None, None)      # orip_gcode_seam accepts P, P: open strokes, seam 0
    assert seam.tolist() == [0, 0] and st["closed"] == 0 and st["travel_before"] == st["travel_after"] == 5 + 85
