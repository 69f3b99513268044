"""--loop-start on the GPU: orip_gcode_seam against the double of tests/seam_double.py -- every seam and all four counts -- on the smallest shapes that can
break the kernels (wave and tile edges, both sides of the hand-over between the two backward kernels, a deep chain, values beyond 32 bits, ties); the
consequences of the rule, which need no double, on a plot too large for comfort; every argument check, with the device still answering afterwards; and
the whole tools, in process and as the scripts on disk, against the host flow run through the doubles and through the stage-14 decoder.  Every comparison
is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import seam_cases as SC
import seam_double as SD
import improve_double as ID
import gcode_double as D
import pens_double as PD
from stream_double import codes_numpy
from test_pens_host import GP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
TOP = 1 << 30
MAP = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=1.0, W=30000, H=30000, invert_y=0)


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def same(dev, case):
    off, pts, order, rev, start = case
    seam, st = dev.gcode_seam(off, pts, order, rev, start)
    want, wst = SD.seams(off, pts, order, rev, start)
    assert seam.dtype == np.int32 and len(seam) == len(off) - 1
    assert np.array_equal(seam, want), (np.nonzero(seam != want)[0][:5], seam[seam != want][:5], want[seam != want][:5], st, wst)
    assert st == wst
    return seam, st


# ------------------------------------------------------------------ equality with the double
def test_nothing_and_one_stroke(dev):
    seam, st = dev.gcode_seam(np.zeros(1, np.int64), np.zeros((0, 2), np.int32), None, None)
    assert len(seam) == 0 and st == dict.fromkeys(SD.STAT_NAMES, 0)
    assert dev.gcode_seam(np.zeros(1, np.int64), np.zeros((0, 2), np.int32), [], [])[1] == dict.fromkeys(SD.STAT_NAMES, 0)
    seam, st = same(dev, SC.pack([SC.line(3, 4, 30, 40)], start=(9, 9)))
    assert st == dict(closed=0, moved=0, travel_before=6, travel_after=6)
    seam, st = same(dev, SC.equidistant())
    assert seam.tolist() == [1] and st == dict(closed=1, moved=1, travel_before=40, travel_after=20)      # vertices 1 and 2 tie: the lower one


def test_all_open_comes_back_as_it_was(dev):
    seam, st = same(dev, SC.all_open())
    assert not seam.any() and st["closed"] == 0 and st["travel_before"] == st["travel_after"]


def test_short_strokes_among_rings(dev):
    seam, st = same(dev, SC.mixed_small())
    assert st["closed"] == 4 and not seam[[1, 3, 5]].any()


@pytest.mark.parametrize("name", sorted(SC.placements()))
def test_where_the_runs_lie(dev, name):
    same(dev, SC.placements()[name])


def test_lattice_ties(dev):
    assert same(dev, SC.lattice())[1]["moved"] > 5


def test_figure_eight(dev):
    seam, st = same(dev, SC.figure_eight())
    assert seam[1] == 0 and st["closed"] == 3


def test_tiny_sequences(dev):
    for seed in range(60):
        same(dev, SC.tiny(seed))


def test_wave_and_chunk_edges(dev):
    assert same(dev, SC.wave_edges())[1]["closed"] == 50


def test_rings_around_one_chunk(dev):
    assert same(dev, SC.chunk_edges())[1]["closed"] == 16


@pytest.mark.parametrize("other", [1023, 1024, 1025])
def test_around_the_hand_over(dev, other):
    assert 1024 * 1023 < SC.HAND_OVER == 1024 * 1024 < 1024 * 1025
    assert same(dev, SC.around_hand_over(other))[1]["moved"] == 4


def test_a_point_next_to_3000(dev):
    same(dev, SC.one_by_3000())


def test_pair_of_3000(dev):
    assert same(dev, SC.pair_3000())[1]["moved"] == 2


def test_large_layers_in_several_runs_and_levels(dev):
    """three large layers on top of each other in one run, one in another: the levels of the backward pass"""
    rng = np.random.default_rng(21)
    big = lambda: SC.ring(int(rng.integers(3000, 9000)), int(rng.integers(3000, 9000)), 1100, 1100, float(rng.uniform(0, 6)))
    small = lambda: SC.ring(int(rng.integers(100, 9000)), int(rng.integers(100, 9000)), 30, 9, float(rng.uniform(0, 6)))
    same(dev, SC.pack([small(), big(), big(), big(), big(), small(), SC.line(5, 5, 9, 9), big(), big(), small(), SC.line(1, 1, 2, 2), small()]))


def test_chain_of_2000_triangles(dev):
    assert same(dev, SC.triangles())[1]["closed"] == 2000


def test_values_beyond_32_bits(dev):
    seam, st = same(dev, SC.far_apart())
    assert st["travel_after"] > 1 << 32
    seam, st = same(dev, SC.corners())
    assert st["travel_before"] > 1 << 32


def test_order_and_directions(dev):
    off, pts, order, rev, start = SC.shuffled()
    same(dev, (off, pts, order, rev, start))
    same(dev, (off, pts, None, None, start))
    same(dev, (off, pts, order, None, start))
    same(dev, (off, pts, None, rev, start))


def test_resident_form(dev):
    off0, pts0, order, rev, start = SC.shuffled()
    off, pts = dev.gcode_to_steps(off0, pts0.astype(np.float64), MAP)
    assert np.array_equal(off, off0) and np.array_equal(pts, pts0)
    want = SD.seams(off, pts, order, rev, start)
    for got in (dev.gcode_seam(None, None, order, rev, start, n=len(off) - 1), dev.gcode_seam(off, pts, order, rev, start), dev.gcode_seam(None, None, order, rev, start)):
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    other = SC.lattice()                                                            # an explicit input does not become the resident list
    same(dev, other)
    back = dev.gcode_steps_fetch(len(off) - 1, len(pts))
    assert np.array_equal(back[0], off) and np.array_equal(back[1], pts)
    got = dev.gcode_seam(None, None, order, rev, start)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]


# ------------------------------------------------------------------ the consequences, without the double
def segment_keys(off, pts):
    """per stroke, the sorted undirected segments as one array"""
    pts = np.asarray(pts, np.int64)
    key = (pts[:, 0] << 31) | pts[:, 1]
    a, b = key[:-1], key[1:]
    inner = np.ones(len(a), bool); inner[np.asarray(off[1:-1]) - 1] = False
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    stroke = np.repeat(np.arange(len(off) - 1), np.diff(off))[:-1]
    rows = np.stack([stroke, lo, hi], 1)[inner]
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]


def test_consequences_on_3000_rings(dev):
    from orip import gcode as GC
    off, pts = SC.random_rings()
    n = len(off) - 1
    ends = GC.path_ends(off, pts)
    order, rev = dev.gcode_order_pens(ends, np.zeros(n, np.int32), 1, True)
    rev[::7] = True                                                                 # the order has no reason to turn a ring round; its direction is the caller's
    seam, st = dev.gcode_seam(off, pts, order, rev)
    L = np.diff(off)[order]
    assert st["closed"] == n and st["moved"] == int((seam != 0).sum()) > n // 2 and (seam >= 0).all() and (seam < L - 1).all()
    before = GC.gather_paths(off, pts, order, rev)
    goff, gpts = GC.gather_paths(off, pts, order, rev, seam)
    assert st["travel_before"] == GC.travel_steps(*before) and st["travel_after"] == GC.travel_steps(goff, gpts) < st["travel_before"]
    assert GC.draw_steps(goff, gpts) == GC.draw_steps(*before) and np.array_equal(goff, before[0])
    assert np.array_equal(segment_keys(goff, gpts), segment_keys(*before))         # per stroke the same multiset of segments
    same_pt = (np.diff(gpts.astype(np.int64), axis=0) == 0).all(1)
    assert not np.delete(same_pt, goff[1:-1] - 1).any()                            # no stroke gains a repeated point
    assert np.array_equal(gpts[goff[:-1]], gpts[goff[1:] - 1])                      # still closed
    # idempotent
    again, st2 = dev.gcode_seam(goff, gpts, None, None)
    assert not again.any() and st2 == dict(closed=n, moved=0, travel_before=st["travel_after"], travel_after=st["travel_after"])
    # changing one seam alone never lowers the travel: every vertex of every ring, between its neighbours as they are
    a = gpts[goff[:-1]].astype(np.int64)
    prev = np.concatenate([np.zeros((1, 2), np.int64), a[:-1]]); nxt = np.concatenate([a[1:], a[-1:]])
    stored = pts.astype(np.int64)
    for k in range(n):
        V = stored[off[order[k]]:off[order[k] + 1] - 1]
        cost = np.abs(V - prev[k]).max(1) + (np.abs(V - nxt[k]).max(1) if k + 1 < n else 0)
        assert cost.min() == cost[seam[k]]


# ------------------------------------------------------------------ bad arguments
def raw(dev, off, pts, n, order, rev, start, seam=True, stats=True):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((off, np.int64), (pts, np.int32), (order, np.int32), (rev, np.uint8), (start, np.int32))]
    out_seam = np.full(max(int(n), 1) if 0 <= n < 100 else 1, -7, np.int32); out_st = np.full(4, -7, np.int64)
    rc = dev.L.orip_gcode_seam(dev.h, p(keep[0]), p(keep[1]), int(n), p(keep[2]), p(keep[3]), p(keep[4]), p(out_seam) if seam else None, p(out_st) if stats else None)
    assert rc == 0 or ((out_seam == -7).all() and (out_st == -7).all())             # a refused call touches nothing
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def test_bad_arguments(dev):
    from orip.device import OripError
    off = np.array([0, 5, 7, 12]); pts = np.concatenate([SC.square(0, 0, 9), SC.line(20, 20, 30, 30), SC.square(40, 0, 9)])
    o = np.array([2, 0, 1]); r = np.array([0, 1, 0]); s = np.array([0, 0])
    def with_pt(i, j, v):
        q = pts.copy(); q[i, j] = v
        return q
    bad = [("n < 0", (off, pts, -1, o, r, s)), ("n > 2^26", (off, pts, (1 << 26) + 1, o, r, s)), ("off not from 0", (off + 1, pts, 3, o, r, s)),
           ("a stroke of one point", (np.array([0, 5, 6, 12]), pts, 3, o, r, s)), ("offsets decrease", (np.array([0, 7, 5, 12]), pts, 3, o, r, s)),
           ("off without pts", (off, None, 3, o, r, s)), ("pts without off", (None, pts, 3, o, r, s)),
           ("x < 0", (off, with_pt(1, 0, -1), 3, o, r, s)), ("y > 2^30", (off, with_pt(6, 1, TOP + 1), 3, o, r, s)),
           ("start < 0", (off, pts, 3, o, r, np.array([-1, 0]))), ("start > 2^30", (off, pts, 3, o, r, np.array([0, TOP + 1]))),
           ("not a permutation", (off, pts, 3, np.array([0, 2, 2]), r, s)), ("an index out of range", (off, pts, 3, np.array([0, 3, 1]), r, s)),
           ("a negative index", (off, pts, 3, np.array([0, -1, 1]), r, s)), ("rev of 2", (off, pts, 3, o, np.array([0, 2, 0]), s))]
    for what, args in bad:
        rc, msg = raw(dev, *args)
        assert rc != 0 and "orip_gcode_seam" in msg, what
    for kw in (dict(seam=False), dict(stats=False)):
        rc, msg = raw(dev, off, pts, 3, o, r, s, **kw)
        assert rc != 0 and "orip_gcode_seam" in msg
    got_off, _ = dev.gcode_to_steps(np.array([0, 2, 4]), np.array([[0.0, 0.0], [5.0, 1.0], [2.0, 2.0], [3.0, 3.0]]), MAP)
    assert len(got_off) == 3
    rc, msg = raw(dev, None, None, 3, o, r, s)                                      # three asked for, two resident
    assert rc != 0 and "resident" in msg
    assert raw(dev, off, pts, 3, o, r, s)[0] == 0 and raw(dev, off, pts, 3, None, None, None)[0] == 0      # and the same call without a fault is taken
    assert np.array_equal(dev.gcode_steps_fetch(2, 4)[0], got_off)                  # the resident list is what it was
    for kw in (dict(order=[0, 0, 1]), dict(rev=[0, 3, 0]), dict(start=(-1, 0)), dict(order=[0, 1])):
        args = dict(order=o, rev=r, start=(0, 0)); args.update(kw)
        with pytest.raises((OripError, ValueError)):
            dev.gcode_seam(off, pts, args["order"], args["rev"], args["start"])
    with pytest.raises(OripError):
        dev.gcode_seam(None, None, o, r, n=3)
    got = dev.gcode_seam(off, pts, o, r)
    want = SD.seams(off, pts, o, r)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]


# ------------------------------------------------------------------ the whole tools
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)
SEAM = dict(seam_fn=lambda off, pts, order, rev: SD.seams(off, pts, order, rev, (0, 0)))
IMPROVE = dict(improve_fn=lambda ends, group, n_groups, order, rev, reverse, max_rounds: ID.improve(ends, group, n_groups, order, rev, reverse, (0, 0), max_rounds))


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def decode(dev, data, info):
    from orip import stream_preview as SP
    W, H = info["target"]
    return SP.preview(dev, data, W, H, 320, 240, invert_y=True)[1]


def run(script, args):
    return subprocess.run([sys.executable, os.path.join(SCRIPTS, script)] + args, capture_output=True, text=True, timeout=300)


def decoded_as_the_rule_says(dev, got, info, plain, pinfo):
    saved = info["seam"]["travel_before"] - info["seam"]["travel_after"]
    st, pst = decode(dev, got, info), decode(dev, plain, pinfo)
    assert saved > 0 and st["steps_total"] == pst["steps_total"] - saved == info["steps"]
    assert st["pen_down_segments"] == pst["pen_down_segments"] and st["color_changes"] == pst["color_changes"] and st["eof_seen"] == 1 and st["off_canvas_draws"] == 0


def test_svg_tool(dev, tmp_path):
    from orip import svg as SV, gcode as GC
    args = SC.TOOL_SVG_ARGS + ["--improve-order", "--loop-start"]
    want, winfo = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(args), **dict(PD.pens_doubles(), **IMPROVE, **SEAM))
    got, info = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(args), dev)
    assert got == want and info["seam"] == winfo["seam"] and info["improve"] == winfo["improve"] and info["pens"] == winfo["pens"]
    assert info["seam"]["travel_before"] == info["improve"]["travel_after"] and info["seam"]["closed"] == 12
    plain, pinfo = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(args[:-1]), dev)
    decoded_as_the_rule_says(dev, got, info, plain, pinfo)
    src = tmp_path / "drawing.svg"
    src.write_bytes(SC.TOOL_SVG)
    r = run("svg2stream.py", [str(src), "--no-preview"] + args)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "drawing_stream.bin").read_bytes() == want and GC.seam_line("svg", info["seam"]) in r.stdout
    gcode_with = (tmp_path / "drawing.gcode").read_text()
    r = run("svg2stream.py", [str(src), "--no-preview"] + args[:-1])
    assert r.returncode == 0 and (tmp_path / "drawing.gcode").read_text() == gcode_with and "loop start" not in r.stdout      # the G-code file is unchanged
    r = run("svg2gcode.py", [str(src), "-o", str(tmp_path / "x.gcode"), "--loop-start"])
    assert r.returncode != 0                                                        # svg2gcode.py does not get the option


def test_gcode_tool(dev, tmp_path):
    from orip import gcode as GC
    text = SC.tool_gcode()
    for kw in (dict(), dict(no_reorder=True), dict(improve_order=True), dict(merge_paths=True, simplify_mm=0.0)):
        dbl = dict(GCODE_DOUBLES, **IMPROVE, **SEAM)
        if "merge_paths" in kw:
            import merge_double as MD
            import simplify_double as SPD
            dbl = dict(dbl, merge_fn=MD.merge_numpy, simplify_fn=SPD.simplify_numpy)
        want, winfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(loop_start=True, **kw), **dbl)
        got, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(loop_start=True, **kw), dev)
        assert got == want and info["seam"] == winfo["seam"] and info["seam"]["closed"] == 20, kw
        if "improve_order" in kw:
            assert info["seam"]["travel_before"] == info["improve"]["travel_after"]
        plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(**kw), dev)
        assert "seam" not in pinfo
        decoded_as_the_rule_says(dev, got, info, plain, pinfo)
    (tmp_path / "drawing.gcode").write_text(text)
    want, winfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(loop_start=True), **dict(GCODE_DOUBLES, **SEAM))
    r = run("gcode2stream.py", [str(tmp_path / "drawing.gcode"), "-o", str(tmp_path / "out.bin"), "--loop-start"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "out.bin").read_bytes() == want and GC.seam_line("gcode", winfo["seam"]) in r.stdout
    want, winfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(loop_start=True, no_reorder=True), **dict(GCODE_DOUBLES, **SEAM))
    r = run("gcode2stream.py", [str(tmp_path / "drawing.gcode"), "-o", str(tmp_path / "file_order.bin"), "--loop-start", "--no-reorder"])
    assert r.returncode == 0 and (tmp_path / "file_order.bin").read_bytes() == want and GC.seam_line("gcode", winfo["seam"]) in r.stdout


def test_tool_unchanged_without_the_option(dev):
    from orip import svg as SV
    got, info = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PLAIN_ARGS), dev)
    assert got == bytes(GP["tool_plain_stream"]) and "seam" not in info
