"""--improve-order on the GPU: orip_gcode_improve against the brute-force double of tests/improve_double.py -- order, directions and all five counts --
on the smallest shapes that can break the kernel, each with and without reversal; invariants that need no double on a plot too large for it; a group
over the limit; every argument check, with the device still answering afterwards; and the whole tools, in process and as the scripts on disk, against
the host flow run through the doubles and through the stage-14 decoder.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import improve_cases as IC
import improve_double as ID
import gcode_double as D
import pens_double as PD
from stream_double import codes_numpy
from test_pens_host import GP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
TOP = 1 << 30


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def same(dev, case, reverse, max_rounds=None):
    ends, group, ng, order, rev, start = case
    o, r, st = dev.gcode_improve(ends, group, ng, order, rev, reverse, start, max_rounds)
    wo, wr, wst = ID.improve(ends, group, ng, order, rev, reverse, start, max_rounds)
    assert o.dtype == np.int32 and r.dtype == bool and len(o) == len(r) == len(order)
    assert np.array_equal(o, wo) and np.array_equal(r, wr), (reverse, max_rounds, np.nonzero((o != wo) | (r != wr))[0][:5], st, wst)
    assert st == wst
    return st


# ------------------------------------------------------------------ equality with the double
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("m", [0, 1, 2, 3, 4])
def test_tiny(dev, m, reverse):
    same(dev, IC.tiny(m, reverse), reverse)


def test_identical_strokes(dev):
    for reverse in (False, True):
        st = same(dev, IC.identical(), reverse)
        assert st["rounds"] == 0 and st["converged_groups"] == 1


@pytest.mark.parametrize("reverse", [False, True])
def test_lattice_ties(dev, reverse):
    assert same(dev, IC.lattice(reverse), reverse)["rounds"] > 5


@pytest.mark.parametrize("name", sorted(IC.FIRST_MOVES))
def test_crafted_first_moves(dev, name):
    case, reverse, move = IC.FIRST_MOVES[name]
    trace = []
    ID.improve(*case[:5], reverse, case[5], 1, trace=trace)
    assert trace[0][2:] == move
    assert same(dev, case, reverse, 1)["rounds"] == 1
    same(dev, case, reverse)


@pytest.mark.parametrize("reverse", [False, True])
def test_gains_beyond_int32(dev, reverse):
    st = same(dev, IC.corners(reverse), reverse)
    assert st["travel_before"] > 1 << 32 and st["rounds"] > 0


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("m", [63, 64, 65, 257])
def test_wave_and_tile_edges(dev, m, reverse):
    same(dev, IC.random_plot(m, 20 + m, size=600, longest=60, reverse=reverse), reverse, 12)


@pytest.fixture(scope="module")
def greedy_300():
    """random m = 300 from its greedy order, as the tools call it"""
    out = {}
    for reverse in (False, True):
        ends, group, ng, _, _, start = IC.random_plot(300, 31)
        order, rev = PD.order_pens_numpy(ends, group, ng, reverse, start)
        out[reverse] = ((ends, group, ng, order, rev, start), ID.improve(ends, group, ng, order, rev, reverse, start))
    return out


@pytest.mark.parametrize("reverse", [False, True])
def test_random_300_uncapped(dev, greedy_300, reverse):
    (ends, group, ng, order, rev, start), (wo, wr, wst) = greedy_300[reverse]
    o, r, st = dev.gcode_improve(ends, group, ng, order, rev, reverse, start)
    assert np.array_equal(o, wo) and np.array_equal(r, wr) and st == wst
    assert st["converged_groups"] == 1 and 20 < st["rounds"] < 300 and st["travel_after"] < 0.9 * st["travel_before"]


@pytest.mark.parametrize("reverse", [False, True])
def test_random_1100_several_tiles(dev, reverse):
    assert same(dev, IC.random_plot(1100, 32, reverse=reverse), reverse, 8)["rounds"] == 8


@pytest.mark.parametrize("cap", [0, 1, 2, IC.BATCH - 1, IC.BATCH, IC.BATCH + 1])
def test_caps_around_the_batch(dev, cap):
    case = IC.random_plot(120, 33, reverse=True)
    st = same(dev, case, True, cap)
    assert st["rounds"] == cap and st["converged_groups"] == 0                   # a shuffled plot of 120 strokes needs more than 33 rounds


@pytest.mark.parametrize("reverse", [False, True])
def test_four_groups_and_the_cursor(dev, reverse):
    st = same(dev, IC.four_groups(reverse), reverse)
    assert st["converged_groups"] == 2 and st["travel_before"] > 1 << 29
    same(dev, IC.random_plot(200, 34, n_groups=5, reverse=reverse), reverse, 40)


MAP = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=1.0, W=4000, H=4000, invert_y=0)


def test_resident_form(dev):
    rng = np.random.default_rng(35)
    n = 70
    pts_mm = rng.integers(0, 3000, (2 * n, 2)).astype(np.float64)
    pts_mm[1::2] += (pts_mm[1::2] == pts_mm[::2]).all(1, keepdims=True)          # no stroke without length
    off, pts = dev.gcode_to_steps(np.arange(0, 2 * n + 1, 2), pts_mm, MAP)
    assert len(off) - 1 == n
    ends = np.concatenate([pts[off[:-1]], pts[off[1:] - 1]], 1)
    group = rng.integers(0, 2, n).astype(np.int32)
    order, rev = IC.sequence(group, rng, True)
    want = ID.improve(ends, group, 2, order, rev, True, (5, 5))
    for got in (dev.gcode_improve(None, group, 2, order, rev, True, (5, 5), n=n), dev.gcode_improve(ends, group, 2, order, rev, True, (5, 5))):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


# ------------------------------------------------------------------ invariants that need no double
def test_invariants_on_2000(dev):
    ends, group, ng, _, _, start = IC.random_plot(2000, 36, n_groups=2)
    order, rev = dev.gcode_order_pens(ends, group, ng, True, start)
    o, r, st = dev.gcode_improve(ends, group, ng, order, rev, True, start)
    assert sorted(o.tolist()) == list(range(2000)) and (np.diff(group[o]) >= 0).all()
    assert st["travel_before"] == ID.travel(ends, order, rev, start) and st["travel_after"] == ID.travel(ends, o, r, start)
    assert st["travel_after"] < st["travel_before"] and st["converged_groups"] == 2 and st["skipped_groups"] == 0 and 0 < st["rounds"] < 2 * 2000
    a, b = ID.entries(ends, o, r)
    cursor = np.asarray(start)
    for g in range(ng):
        pos = np.nonzero(group[o] == g)[0]
        assert ID.best_move(a[pos], b[pos], cursor, True)[0] <= 0
        cursor = b[pos[-1]]


# ------------------------------------------------------------------ a group over the limit
def test_skipped_group(dev):
    big = ID.MAX_PATHS + 1
    rng = np.random.default_rng(37)
    e_big = rng.integers(0, 9000, (big, 4)).astype(np.int32)
    small = IC.random_plot(20, 38)
    ends = np.concatenate([e_big, small[0]])
    group = np.concatenate([np.zeros(big, np.int32), np.ones(20, np.int32)])
    order, rev = IC.sequence(group)
    o, r, st = dev.gcode_improve(ends, group, 2, order, rev, False, (0, 0), 4)
    assert np.array_equal(o[:big], order[:big]) and not r.any() and st["skipped_groups"] == 1 and st["rounds"] == 4 and st["converged_groups"] == 0
    cursor = tuple(e_big[-1, 2:].tolist())                                       # the big group ends where it always ended
    wo, wr, wst = ID.improve(small[0], small[1], 1, order[big:] - big, rev[big:], False, cursor, 4)
    assert np.array_equal(o[big:] - big, wo) and st["travel_before"] - st["travel_after"] == wst["travel_before"] - wst["travel_after"] > 0
    assert st["travel_before"] == ID.travel(ends, order, rev)


# ------------------------------------------------------------------ bad arguments
def raw(dev, ends, group, n, n_groups, flags, start, max_rounds, order, rev, stats=True):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = np.full(5, -7, np.int64)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((ends, np.int32), (group, np.int32), (start, np.int32), (order, np.int32), (rev, np.uint8))]
    before = [None if a is None else a.copy() for a in keep]
    rc = dev.L.orip_gcode_improve(dev.h, p(keep[0]), p(keep[1]), int(n), int(n_groups), int(flags), p(keep[2]), int(max_rounds), p(keep[3]), p(keep[4]), p(st) if stats else None)
    assert rc == 0 or all(a is None or np.array_equal(a, b) for a, b in zip(keep, before))      # a refused call touches nothing
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def test_bad_arguments(dev):
    from orip.device import OripError
    e = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 9, 2, 2]]); g = np.array([0, 1, 1]); o = np.array([0, 2, 1]); r = np.array([0, 0, 0]); s = np.array([0, 0])
    good = (e, g, 3, 2, 1, s, 5, o, r)
    bad = [("not a permutation", (e, g, 3, 2, 1, s, 5, np.array([0, 2, 2]), r)), ("an index out of range", (e, g, 3, 2, 1, s, 5, np.array([0, 3, 1]), r)),
           ("a negative index", (e, g, 3, 2, 1, s, 5, np.array([0, -1, 1]), r)), ("groups decrease", (e, g, 3, 2, 1, s, 5, np.array([1, 0, 2]), r)),
           ("rev without the flag", (e, g, 3, 2, 0, s, 5, o, np.array([0, 1, 0]))), ("rev of 2", (e, g, 3, 2, 1, s, 5, o, np.array([0, 2, 0]))),
           ("negative rounds", (e, g, 3, 2, 1, s, -1, o, r)), ("very negative rounds", (e, g, 3, 2, 1, s, -(1 << 62), o, r)),
           ("n < 0", (e, g, -1, 2, 1, s, 5, o, r)), ("n > 2^26", (e, g, (1 << 26) + 1, 2, 1, s, 5, o, r)), ("no groups", (e, g, 3, 0, 1, s, 5, o, r)), ("65 groups", (e, g, 3, 65, 1, s, 5, o, r)),
           ("unknown flags", (e, g, 3, 2, 2, s, 5, o, r)), ("group == n_groups", (e, np.array([0, 1, 2]), 3, 2, 1, s, 5, o, r)), ("group < 0", (e, np.array([0, -1, 1]), 3, 2, 1, s, 5, o, r)),
           ("x < 0", (np.array([[1, 2, 3, 4], [-5, 6, 7, 8], [9, 9, 2, 2]]), g, 3, 2, 1, s, 5, o, r)), ("y > 2^30", (np.array([[1, 2, 3, 4], [5, 6, 7, TOP + 1], [9, 9, 2, 2]]), g, 3, 2, 1, s, 5, o, r)),
           ("start < 0", (e, g, 3, 2, 1, np.array([-1, 0]), 5, o, r)), ("start > 2^30", (e, g, 3, 2, 1, np.array([0, TOP + 1]), 5, o, r)),
           ("group NULL", (e, None, 3, 2, 1, s, 5, o, r)), ("order NULL", (e, g, 3, 2, 1, s, 5, None, r)), ("rev NULL", (e, g, 3, 2, 1, s, 5, o, None))]
    for what, args in bad:
        rc, msg = raw(dev, *args)
        assert rc != 0 and "orip_gcode_improve" in msg, what
    rc, msg = raw(dev, *good, stats=False)
    assert rc != 0 and "orip_gcode_improve" in msg
    off, _ = dev.gcode_to_steps(np.array([0, 2, 4]), np.array([[0.0, 0.0], [5.0, 1.0], [2.0, 2.0], [3.0, 3.0]]), dict(MAP, steps_per_mm=10.0))
    assert len(off) == 3
    rc, msg = raw(dev, None, g, 3, 2, 1, s, 5, o, r)                               # three asked for, two resident
    assert rc != 0 and "resident" in msg
    assert raw(dev, *good)[0] == 0                                                # and the same call without a fault is taken
    for kw in (dict(order=[0, 0, 1]), dict(order=[1, 0, 2]), dict(rev=[1, 0, 0], reverse=False), dict(max_rounds=-3), dict(start=(-1, 0))):
        args = dict(order=o, rev=r, reverse=True, max_rounds=5, start=(0, 0)); args.update(kw)
        with pytest.raises(OripError):
            dev.gcode_improve(e, g, 2, args["order"], args["rev"], args["reverse"], args["start"], args["max_rounds"])
    with pytest.raises(OripError):
        dev.gcode_improve(None, g, 2, o, r, n=3)
    got = dev.gcode_improve(e, g, 2, o, r, True)
    want = ID.improve(e, g, 2, o, r, True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert dev.gcode_improve(np.zeros((0, 4), np.int32), [], 1, [], [])[2] == dict.fromkeys(ID.STAT_NAMES, 0)


# ------------------------------------------------------------------ the whole tools
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)
IMPROVE = dict(improve_fn=lambda ends, group, n_groups, order, rev, reverse, max_rounds: ID.improve(ends, group, n_groups, order, rev, reverse, (0, 0), max_rounds))
SVG_ARGS = PD.TOOL_PEN_ARGS + ["--improve-order"]


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def decode(dev, data, info):
    from orip import stream_preview as SP
    W, H = info["target"]
    return SP.preview(dev, data, W, H, 320, 240, invert_y=True)[1]


def run(script, args):
    return subprocess.run([sys.executable, os.path.join(SCRIPTS, script)] + args, capture_output=True, text=True, timeout=300)


def test_svg_tool(dev, tmp_path):
    from orip import svg as SV, gcode as GC
    want, winfo = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(SVG_ARGS), **dict(PD.pens_doubles(), **IMPROVE))
    got, info = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(SVG_ARGS), dev)
    assert got == want and info["improve"] == winfo["improve"] and info["pens"] == winfo["pens"]
    plain, pinfo = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PEN_ARGS), dev)
    saved = info["improve"]["travel_before"] - info["improve"]["travel_after"]
    st, pst = decode(dev, got, info), decode(dev, plain, pinfo)
    assert saved > 0 and st["steps_total"] == pst["steps_total"] - saved == info["steps"]
    assert st["pen_down_segments"] == pst["pen_down_segments"] and st["color_changes"] == pst["color_changes"] == 4 and st["eof_seen"] == 1 and st["off_canvas_draws"] == 0
    src = tmp_path / "drawing.svg"
    src.write_bytes(PD.TOOL_SVG)
    r = run("svg2stream.py", [str(src), "--no-preview"] + SVG_ARGS)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "drawing_stream.bin").read_bytes() == want and GC.improve_line("svg", info["improve"]) in r.stdout


def test_gcode_tool(dev, tmp_path):
    from orip import gcode as GC
    text = IC.tool_gcode()
    want, winfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(improve_order=True), **dict(GCODE_DOUBLES, **IMPROVE))
    got, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(improve_order=True), dev)
    assert got == want and info["improve"] == winfo["improve"] and "reversed" not in info
    plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(), dev)
    saved = info["improve"]["travel_before"] - info["improve"]["travel_after"]
    st, pst = decode(dev, got, info), decode(dev, plain, pinfo)
    assert saved > 0 and st["steps_total"] == pst["steps_total"] - saved == info["steps"]
    assert st["pen_down_segments"] == pst["pen_down_segments"] == 90 and st["color_changes"] == pst["color_changes"] and st["eof_seen"] == 1
    (tmp_path / "drawing.gcode").write_text(text)
    r = run("gcode2stream.py", [str(tmp_path / "drawing.gcode"), "-o", str(tmp_path / "out.bin"), "--improve-order"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "out.bin").read_bytes() == want and GC.improve_line("gcode", info["improve"]) in r.stdout
    r = run("gcode2stream.py", [str(tmp_path / "drawing.gcode"), "-o", str(tmp_path / "no.bin"), "--improve-order", "--no-reorder"])
    assert r.returncode != 0 and not (tmp_path / "no.bin").exists()


def test_tool_unchanged_without_the_option(dev):
    from orip import svg as SV
    got, info = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PLAIN_ARGS), dev)
    assert got == bytes(GP["tool_plain_stream"]) and "improve" not in info
