"""The dash pass on the GPU: orip_gcode_dash against the sequential double of tests/dash_double.py -- off, pts, origin and all eight stats -- on every named
drawing of tests/dash_cases.py and on random drawings; the resident form behind the conversion and behind the clip, where sources repeat; the uploaded form
and what the sources say then; every argument check, with the resident polylines left as they were; and both tools against the host flow run through the
doubles.  No comparison has a tolerance.  The two overflow errors (a stroke of 2^62 units, 2^30 output points) would need giant allocations to provoke and
are not provoked: they are covered by the argument checks around them and by reading csrc/gcode_dash.hip."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dash_cases as DC
import dash_double as DD
import gcode_double as D
import pens_double as PD
from stream_double import codes_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
TOP, U = 1 << 30, 256
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
    assert got[3] == want[3], (got[3], want[3])
    for k, (a, b) in enumerate(zip(got[:3], want[:3])):
        assert a.shape == b.shape and np.array_equal(a, b), (k, a[:8], b[:8])


# ------------------------------------------------------------------ every drawing against the double
def test_nothing_to_dash(dev):
    po, pv = DC.table([DC.ON_OFF])
    got = dev.gcode_dash(np.zeros(1, np.int64), np.zeros((0, 2), np.int32), [], [], po, pv)
    equal(got, DD.dash_numpy([0], np.zeros((0, 2)), [], [], po, pv))
    assert all(v == 0 for v in got[3].values())
    off, pts = dev.gcode_steps_fetch(0, 0)
    assert off.tolist() == [0] and len(pts) == 0
    got = dev.gcode_dash(np.zeros(1, np.int64), np.zeros((0, 2), np.int32), [], [], [0], [])      # and no pattern at all
    assert got[3]["paths_out"] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_shape(dev, name):
    case = CASES[name]
    want = DD.dash_numpy(*case)
    got = dev.gcode_dash(*case)
    equal(got, want)
    f_off, f_pts = dev.gcode_steps_fetch(len(want[0]) - 1, len(want[1]))          # the result is the resident list
    assert np.array_equal(f_off, want[0]) and np.array_equal(f_pts, want[1])


def test_solid_strokes_pass_through(dev):
    off, pts, pattern, phase, po, pv = CASES["mixed_patterns"]
    got = dev.gcode_dash(off, pts, np.full(len(pattern), -1, np.int32), phase * 0, po, pv)
    assert np.array_equal(got[0], off) and np.array_equal(got[1], pts) and np.array_equal(got[2], np.arange(len(off) - 1))
    assert got[3] == dict(paths_in=len(off) - 1, dashed=0, dashes=0, collapsed=0, paths_out=len(off) - 1, points_out=len(pts), length_in=0, length_on=0)


def test_random_drawings(dev):
    for seed in range(300):
        case = DC.random_drawing(seed)
        equal(dev.gcode_dash(*case), DD.dash_numpy(*case))


def test_many_random_strokes_in_one_call(dev):
    """the random drawings side by side in one call with all their patterns: more than one block, every kind of stroke next to every other"""
    lists, pattern, phase, patterns = [], [], [], []
    for seed in range(400):
        off, pts, pa, ph, po, pv = DC.random_drawing(1000 + seed)
        lists += [pts[a:b].tolist() for a, b in zip(off[:-1], off[1:])]
        pattern += [int(q) + len(patterns) if q >= 0 else -1 for q in pa]; phase += ph.tolist()
        patterns += [pv[a:b].tolist() for a, b in zip(po[:-1], po[1:])]
    case = DC.drawing(lists, pattern, phase, patterns)
    equal(dev.gcode_dash(*case), DD.dash_numpy(*case))


# ------------------------------------------------------------------ the resident form
def resident_input(dev, clip=None):
    """a drawing in mm on a grid of one step per mm: a square, a path the conversion drops, an oblique stroke, a long line that leaves a clip rectangle twice"""
    lists = [[(10, 10), (30, 10), (30, 30), (10, 30), (10, 10)], [(50, 50), (50, 50.2)], [(5, 60), (45, 71)], [(0, 20), (60, 20), (60, 25), (0, 25)]]
    off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
    mm = np.asarray([q for p in lists for q in p], np.float64)
    if clip is None:
        return dev.gcode_to_steps(off, mm, MAP)
    return dev.gcode_to_steps_clip(off, mm, MAP, clip)[:2]


def path_patterns(src):
    """pattern and phase per stroke from those of the input paths, as orip.gcode takes them through the sources"""
    pattern, phase = np.array([0, 0, -1, 1], np.int32), np.array([0, 0, 0, 3 * U + 5], np.int64)
    return pattern[src], phase[src]


@pytest.mark.parametrize("clip", [None, (0, 0, 40, 3999)])
def test_resident_form_and_the_sources(dev, clip):
    off, pts = resident_input(dev, clip)
    n = len(off) - 1
    src = dev.gcode_steps_source(n)
    assert src.tolist() == [0, 2, 3] if clip is None else len(set(src.tolist())) < n       # behind the clip the sources repeat
    pattern, phase = path_patterns(src)
    po, pv = DC.table([DC.ON_OFF, DC.WHOLE])
    want = DD.dash_numpy(off, pts, pattern, phase, po, pv)
    got = dev.gcode_dash(None, None, pattern, phase, po, pv, n=n)
    equal(got, want)
    k = len(want[0]) - 1
    assert k > n
    f_off, f_pts = dev.gcode_steps_fetch(k, len(want[1]))
    assert np.array_equal(f_off, want[0]) and np.array_equal(f_pts, want[1])
    assert dev.gcode_steps_source(k).tolist() == src[want[2]].tolist()            # the input path of every dash, gathered through origin
    assert np.array_equal(dev.gcode_order(None, n=k), D.order_numpy(np.concatenate([want[1][want[0][:-1]], want[1][want[0][1:] - 1]], 1)))
    again = dev.gcode_dash(None, None, np.full(k, -1, np.int32), np.zeros(k, np.int64), po, pv, n=k)      # the resident result, all solid: nothing changes
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1]) and np.array_equal(again[2], np.arange(k))
    assert dev.gcode_steps_source(k).tolist() == src[want[2]].tolist()


def test_uploaded_form_and_the_sources(dev):
    from orip.device import OripError
    case = CASES["wholly_in_a_gap"]                                               # 3 strokes, as many as the conversion leaves
    want = DD.dash_numpy(*case)
    rc = dev.L.orip_gcode_to_steps(dev.h, None, None, 0, None, None, None)        # the conversion drops the list before it looks at its arguments
    assert rc != 0
    equal(dev.gcode_dash(*case), want)                                            # no list resident: the strokes have no sources
    with pytest.raises(OripError):
        dev.gcode_steps_source(len(want[0]) - 1)
    r_off, _ = resident_input(dev)
    assert len(r_off) - 1 == len(case[0]) - 1 == 3
    src = dev.gcode_steps_source(3)
    equal(dev.gcode_dash(*case), want)                                            # the resident count: taken for the polylines a fetch gave out
    assert dev.gcode_steps_source(len(want[0]) - 1).tolist() == src[want[2]].tolist()
    resident_input(dev)
    other = CASES["dash_longer_than_the_stroke"]                                  # another count: the sources do not name these
    equal(dev.gcode_dash(*other), DD.dash_numpy(*other))
    with pytest.raises(OripError):
        dev.gcode_steps_source(2)
    resident_input(dev)
    assert dev.gcode_steps_source(3).tolist() == [0, 2, 3]                        # and the next conversion names its sources again


# ------------------------------------------------------------------ bad arguments
def raw(dev, off, pts, pattern, phase, n, pat_off, pat_val, n_patterns, stats=True):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = np.full(8, -7, np.int64)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((off, np.int64), (pts, np.int32), (pattern, np.int32), (phase, np.int64), (pat_off, np.int32),
                                                                             (pat_val, np.int64))]
    rc = dev.L.orip_gcode_dash(dev.h, p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), int(n), p(keep[4]), p(keep[5]), int(n_patterns), p(st) if stats else None)
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def test_bad_arguments_leave_the_resident_paths(dev):
    off0, pts0 = resident_input(dev)
    n0, t0 = len(off0) - 1, len(pts0)
    src0 = dev.gcode_steps_source(n0)
    o = np.array([0, 2, 5]); p = np.array([[1, 1], [2, 2], [2, 2], [3, 3], [9, 3]]); a = np.array([0, 1]); h = np.array([0, 5])
    qo = np.array([0, 2, 6]); qv = np.array([512, 256, 300, 400, 500, 1 << 40])
    A = np.array
    bad = [("n < 0", (o, p, a, h, -1, qo, qv, 2)), ("n > 2^26", (o, p, a, h, (1 << 26) + 1, qo, qv, 2)), ("2^28 points", (A([0, 2, 1 << 28]), p, a, h, 2, qo, qv, 2)),
           ("off[0] != 0", (A([1, 2, 5]), p, a, h, 2, qo, qv, 2)), ("off decreases", (A([0, 3, 2]), p, a, h, 2, qo, qv, 2)), ("a path of one point", (A([0, 4, 5]), p, a, h, 2, qo, qv, 2)),
           ("x < 0", (o, A([[1, 1], [2, 2], [-1, 2], [3, 3], [9, 3]]), a, h, 2, qo, qv, 2)), ("y > 2^30", (o, A([[1, 1], [2, 2], [2, 2], [3, TOP + 1], [9, 3]]), a, h, 2, qo, qv, 2)),
           ("a point twice", (o, A([[1, 1], [2, 2], [2, 2], [3, 3], [3, 3]]), a, h, 2, qo, qv, 2)),
           ("pattern < -1", (o, p, A([0, -2]), h, 2, qo, qv, 2)), ("pattern == np", (o, p, A([0, 2]), h, 2, qo, qv, 2)), ("pattern 0 of none", (o, p, A([0, -1]), h, 2, A([0]), None, 0)),
           ("phase < 0", (o, p, a, A([-1, 0]), 2, qo, qv, 2)), ("phase == P", (o, p, a, A([768, 0]), 2, qo, qv, 2)),
           ("np < 0", (o, p, a, h, 2, qo, qv, -1)), ("np > 2^20", (o, p, a, h, 2, qo, qv, (1 << 20) + 1)),
           ("an odd pattern", (o, p, a, h, 2, A([0, 3, 6]), qv, 2)), ("an empty pattern", (o, p, a, h, 2, A([0, 0, 6]), qv, 2)), ("66 entries", (o, p, A([0, 0]), h, 2, A([0, 66]), np.full(66, 300), 1)),
           ("an entry under a step", (o, p, a, h, 2, qo, A([512, 255, 300, 400, 500, 600]), 2)), ("an entry over 2^40", (o, p, a, h, 2, qo, A([512, 256, 300, 400, 500, (1 << 40) + 1]), 2)),
           ("a negative entry", (o, p, a, h, 2, qo, A([512, 256, -300, 400, 500, 600]), 2)),
           ("pat_off[0] != 0", (o, p, a, h, 2, A([2, 4, 6]), qv, 2)), ("pat_off decreases", (o, p, a, h, 2, A([0, 4, 2]), qv, 2)),
           ("pts NULL", (o, None, a, h, 2, qo, qv, 2)), ("off NULL", (None, p, a, h, 2, qo, qv, 2)), ("pattern NULL", (o, p, None, h, 2, qo, qv, 2)), ("phase NULL", (o, p, a, None, 2, qo, qv, 2)),
           ("pat_off NULL", (o, p, a, h, 2, None, qv, 2)), ("pat_val NULL", (o, p, a, h, 2, qo, None, 2)),
           ("not the resident count", (None, None, a, h, n0 + 1, qo, qv, 2)), ("not the resident count", (None, None, a, h, 0, qo, qv, 2))]
    for what, args in bad:
        rc, msg = raw(dev, *args)
        assert rc != 0 and "orip_gcode_dash" in msg, what
    rc, msg = raw(dev, o, p, a, h, 2, qo, qv, 2, stats=False)
    assert rc != 0 and "orip_gcode_dash" in msg
    off1, pts1 = dev.gcode_steps_fetch(n0, t0)
    assert np.array_equal(off1, off0) and np.array_equal(pts1, pts0) and np.array_equal(dev.gcode_steps_source(n0), src0)
    rc, msg = raw(dev, o, p, a, h, 2, qo, qv, 2)                                  # and the same arguments without a fault are taken
    assert rc == 0, msg
    from orip.device import OripError
    with pytest.raises(OripError):
        dev._ck(dev.L.orip_gcode_dash_fetch(dev.h, None))                         # a result of some strokes and nowhere to put it


# ------------------------------------------------------------------ the whole tools
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)


def run(script, args):
    return subprocess.run([sys.executable, os.path.join(SCRIPTS, script)] + args, capture_output=True, text=True, timeout=300)


def test_gcode_tool(dev, tmp_path):
    from orip import gcode as GC
    opts = GC.options_from_args(GC.build_argparser().parse_args(["in.gcode"] + DC.TOOL_GCODE_ARGS))
    S = PD.StepsWithSource()
    want, winfo = GC.build_stream_from_gcode(DC.TOOL_GCODE, opts, **dict(GCODE_DOUBLES, steps_fn=S.steps, source_fn=S.source, dash_fn=DD.dash_numpy))
    got, info = GC.build_stream_from_gcode(DC.TOOL_GCODE, opts, dev)
    assert got == want and info["dash"] == winfo["dash"] and info["paths"] == winfo["paths"] and info["dash"]["dashes"] > 30
    (tmp_path / "in.gcode").write_text(DC.TOOL_GCODE)
    r = run("gcode2stream.py", [str(tmp_path / "in.gcode"), "-o", str(tmp_path / "out.bin")] + DC.TOOL_GCODE_ARGS)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "out.bin").read_bytes() == want and "[gcode] dash: 3 strokes dashed" in r.stdout


def test_svg_flow_with_the_occlusion_and_the_dedup_behind_the_pass(dev):
    """the residency chain on the device: conversion, dash, occlusion, dedup and merge, each on the polylines the one before it left"""
    from orip import svg as SV
    import clip_double as CD
    import dedup_double as DDD
    import occlude_cases as OC
    text = DC.TOOL_SVG.replace(b'<rect x="5" y="5" width="90" height="70" stroke="black" fill="none"/>', b'<rect x="40" y="5" width="20" height="70" stroke="black" fill="white"/>')
    for extra in ([], ["--clip", "--pen-colors", "#000,#f00", "--merge-paths"]):
        o = SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview", "--dashes", "--occlude", "--dedup"] + extra))
        want, winfo = SV.build_stream_from_svg(text, o, **dict(CD.svg_doubles(), dash_fn=DD.dash_numpy, occlude_fn=OC.OccludeDouble(), dedup_fn=DDD.dedup_numpy))
        got, info = SV.build_stream_from_svg(text, o, dev)
        assert got == want and info["dash"] == winfo["dash"] and info["occlude"] == winfo["occlude"] and info["dedup"] == winfo["dedup"] and info["paths"] == winfo["paths"]
        assert info["occlude"]["hidden"] + info["occlude"]["cut"] > 0


def test_svg_tool(dev, tmp_path):
    from orip import svg as SV
    o = SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + DC.TOOL_SVG_ARGS))
    want, winfo = SV.build_stream_from_svg(DC.TOOL_SVG, o, **dict(PD.pens_doubles(), dash_fn=DD.dash_numpy))
    got, info = SV.build_stream_from_svg(DC.TOOL_SVG, o, dev)
    assert got == want and info["dash"] == winfo["dash"] and info["dash"]["dashed"] == 3 and info["dash"]["ignored"] == 0
    src = tmp_path / "drawing.svg"
    src.write_bytes(DC.TOOL_SVG)
    r = run("svg2stream.py", [str(src), "--no-preview"] + DC.TOOL_SVG_ARGS)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "drawing_stream.bin").read_bytes() == want and "[svg] dash: 3 strokes dashed" in r.stdout
