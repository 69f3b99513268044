"""--ring-entry on the GPU: orip_gcode_order_rings against the double of tests/ring_entry_double.py -- the order, the directions, the seams and all four
counts -- on the smallest inputs that can break the kernel (ties everywhere, the edges of the removal 64 at a time, a crowded cell, cells that hold only
removed candidates, degenerate boxes, groups); against the device's own plain orders where no stroke is closed; the invariants, which need no double, on
10^4 circles; every argument check, with the device still answering afterwards; and the whole tools, in process and as the scripts on disk, against the host
flow run through the doubles and through the stage-14 decoder.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import seam_cases as SC
import seam_double as SD
import ring_entry_double as RD
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


def same(dev, strokes, group=None, n_groups=1, start=(0, 0), both=True):
    """the device's answer is the double's, without and with ORIP_ORDER_REVERSE"""
    off, pts, _, _, _ = SC.pack(strokes)
    out = None
    for reverse in ((False, True) if both else (False,)):
        order, rev, seam, st = dev.gcode_order_rings(off, pts, group, n_groups, reverse, start)
        w_order, w_rev, w_seam, w_st = RD.order_rings(off, pts, group, n_groups, reverse, start)
        assert order.dtype == np.int32 and seam.dtype == np.int32 and rev.dtype == bool and len(order) == len(rev) == len(seam) == len(off) - 1
        bad = np.nonzero((order != w_order) | (rev != w_rev) | (seam != w_seam))[0]
        assert len(bad) == 0, (reverse, bad[:5], order[bad[:5]], w_order[bad[:5]], seam[bad[:5]], w_seam[bad[:5]], st, w_st)
        assert st == w_st, reverse
        out = out or (order, rev, seam, st)
    return out


# ------------------------------------------------------------------ equality with the double
def test_nothing_one_stroke_one_ring(dev):
    order, rev, seam, st = dev.gcode_order_rings(np.zeros(1, np.int64), np.zeros((0, 2), np.int32), None, 1)
    assert len(order) == len(rev) == len(seam) == 0 and st == dict.fromkeys(RD.STAT_NAMES, 0)
    assert dev.gcode_order_rings(np.zeros(1, np.int64), np.zeros((0, 2), np.int32), [], 5, True, (7, 7))[3] == dict.fromkeys(RD.STAT_NAMES, 0)
    _, _, _, st = same(dev, [SC.line(3, 4, 30, 40)], start=(9, 9))
    assert st == dict(closed=0, moved=0, candidates=1, travel=6)
    off, pts, _, _, start = SC.equidistant()
    order, rev, seam, st = dev.gcode_order_rings(off, pts, None, 1, False, start)
    assert seam.tolist() == [1] and st == dict(closed=1, moved=1, candidates=4, travel=20)      # vertices 1 and 2 tie in L1: the lower one
    same(dev, [np.array([[5, 5]])], start=(2, 9))                                                # one dot


def test_smallest_closed_stroke_beside_open_ones(dev):
    tri = np.array([[10, 10], [20, 10], [15, 20], [10, 10]])                                     # 4 points: the smallest closed stroke
    aba = np.array([[12, 12], [30, 30], [12, 12]])                                               # A, B, A is open
    aa = np.array([[40, 40], [40, 40]])
    dots = [np.array([[x, y]]) for x, y in ((10, 10), (15, 20), (41, 41), (0, 0))]
    order, rev, seam, st = same(dev, [tri, aba, aa] + dots + [tri + 30], start=(16, 19))
    assert st["closed"] == 2 and st["candidates"] == 3 + 1 + 1 + 4 + 3
    assert same(dev, [aba, tri, aba[::-1]], start=(29, 29))[3]["closed"] == 1


def test_hand_worked_cases(dev):
    a = np.array([[20, 20], [10, 20], [10, 10], [20, 10], [20, 20]])
    b = np.array([[50, 20], [40, 20], [40, 10], [50, 10], [50, 20]])
    order, rev, seam, st = same(dev, [a, b])
    assert (order.tolist(), seam.tolist()) == ([0, 1], [2, 2]) and st == dict(closed=2, moved=2, candidates=8, travel=40)
    order, rev, seam, st = same(dev, [SC.square(30, 30, 10), SC.square(5, 5, 10), SC.square(30, 30, 10)])      # two coincident rings
    assert order.tolist() == [1, 0, 2] and seam.tolist() == [0, 0, 0]
    off, pts, _, _, _ = SC.figure_eight()
    order, rev, seam, st = same(dev, SD.strokes_of(off, pts))
    assert order.tolist() == [0, 1, 2, 3] and seam.tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("block", range(3))
def test_tiny_sequences_on_a_coarse_lattice(dev, block):
    some_closed = 0
    for seed in range(20 * block, 20 * block + 20):
        off, pts, _, _, start = SC.tiny(seed)
        rng = np.random.default_rng(1000 + seed)
        strokes = SD.strokes_of(off, pts) + [rng.integers(0, 6, (1, 2)) for _ in range(int(rng.integers(0, 3)))]
        grp = rng.integers(0, 2, len(strokes)).astype(np.int32)
        some_closed += same(dev, strokes, grp, 2, start)[3]["closed"] > 0
        same(dev, strokes, None, 1, start)
    assert some_closed > 8


def lattice_case(seed, n=40):
    """squares, A, B, A, lines and dots on a lattice of pitch 10: most candidates tie"""
    rng = np.random.default_rng(seed)
    strokes = []
    for x, y, kind in zip(rng.integers(0, 6, n), rng.integers(0, 6, n), rng.integers(0, 4, n)):
        x, y = 10 * int(x), 10 * int(y)
        strokes.append([np.roll(SC.square(x, y, 10)[:-1], int(rng.integers(0, 4)), 0), np.array([[x, y], [x + 10, y]]), np.array([[x, y], [x, y + 10], [x, y]]), np.array([[x, y]])][kind])
        if kind == 0:
            strokes[-1] = np.concatenate([strokes[-1], strokes[-1][:1]])
    return strokes, rng.integers(0, 3, n).astype(np.int32)


@pytest.mark.parametrize("seed", range(4))
def test_ties_everywhere(dev, seed):
    strokes, grp = lattice_case(seed)
    assert same(dev, strokes, None, 1, (25, 25))[3]["closed"] > 3
    same(dev, strokes, grp, 3, (25, 25))


@pytest.mark.parametrize("m", [63, 64, 65, 129])
def test_rings_at_the_edges_of_the_removal(dev, m):
    """a ring of m vertices leaves 64 candidates at a time; the open strokes inside and beside it must find none of them afterwards"""
    r = 2 * m
    big = SC.ring(3 * r, 3 * r, r, m, 0.4)
    inside = [SC.line(3 * r + dx, 3 * r + dy, 3 * r + dx + 3, 3 * r + dy + 2) for dx, dy in ((0, 0), (r - 9, 0), (0, r - 9), (-r + 9, 5), (7, -r + 9))]
    order, rev, seam, st = same(dev, inside[:2] + [big, SC.ring(3 * r, 3 * r, r // 2, m, 1.0)] + inside[2:] + [SC.ring(8 * r, 3 * r, r, m, 2.0)], start=(3 * r, 0))
    assert st["closed"] == 3 and st["candidates"] >= 3 * m


def test_a_crowded_cell_beside_a_ring_over_many_cells(dev):
    """200 ring vertices on a 3 x 3 patch (one cell, scanned by the whole wave) and a ring of 200 over the sheet; lines between them"""
    rng = np.random.default_rng(5)
    p = rng.integers(0, 3, (200, 2)) + 500
    p[1:][(np.diff(p, axis=0) == 0).all(1)] += [[1, 0]]
    crowded = np.concatenate([p, p[:1]])
    wide = SC.ring(2000, 2000, 1500, 200, 0.1)
    lines = [SC.line(int(x), int(y), int(x) + 5, int(y) + 9) for x, y in rng.integers(0, 4000, (30, 2))]
    order, rev, seam, st = same(dev, lines[:15] + [crowded, wide] + lines[15:] + [crowded + 3], start=(490, 505))
    assert st["closed"] == 3 and st["candidates"] == 30 + 600
    same(dev, [crowded, crowded, crowded[::-1]], start=(0, 0), both=False)                       # one cell holds everything


def test_concentric_rings_in_the_same_cells(dev):
    """two rings whose vertices interleave on one circle: one is taken whole, the other stays whole"""
    a, b = SC.ring(300, 300, 200, 40, 0.0), SC.ring(300, 300, 200, 40, np.pi / 40)
    order, rev, seam, st = same(dev, [a, b, SC.line(300, 300, 310, 300), SC.ring(300, 300, 198, 64, 0.05), SC.line(900, 900, 901, 901)], start=(505, 300))
    assert st["closed"] == 3


def test_the_window_grows_through_cells_of_removed_candidates(dev):
    """200 small rings in a cluster and one stroke far away: behind the last ring every cell around the cursor holds only dead entries"""
    rng = np.random.default_rng(6)
    c = rng.integers(20, 400, (200, 2))
    rings = [SC.ring(int(x), int(y), 6, 6, float(t)) for (x, y), t in zip(c, rng.uniform(0, 6, 200))]
    order, rev, seam, st = same(dev, rings[:100] + [SC.line(60000, 50000, 60010, 50000)] + rings[100:], both=False)
    assert order[-1] == 100 and st["closed"] == 200
    grp = np.array([1] * 100 + [0] + [1] * 100, np.int32)                                         # the far stroke first: the cursor comes from far outside the box
    same(dev, rings[:100] + [SC.line(60000, 50000, 60010, 50000)] + rings[100:], grp, 2, both=False)


def test_degenerate_boxes_and_the_ends_of_the_range(dev):
    row = [np.array([[x, 7], [x + 3, 7], [x + 6, 7], [x, 7]]) for x in range(0, 400, 10)] + [SC.line(x, 7, x + 1, 7) for x in range(5, 400, 30)]
    same(dev, row, start=(200, 7))                                                               # every candidate on one row
    same(dev, row, start=(200, TOP))                                                             # and the cursor far outside the box
    same(dev, [s[:, ::-1] for s in row], start=(TOP, 0))                                         # one column
    off, pts, _, _, start = SC.corners()
    same(dev, SD.strokes_of(off, pts), start=start)                                              # coordinates 0 and 2^30 only
    off, pts, _, _, start = SC.far_apart()
    same(dev, SD.strokes_of(off, pts), start=start)
    assert same(dev, SD.strokes_of(off, pts), np.arange(10, dtype=np.int32), 10, start)[3]["travel"] > 1 << 32      # a group each: every approach crosses the range
    same(dev, [SC.square(0, 0, TOP), np.array([[TOP, TOP]]), SC.line(0, TOP, TOP, 0)], start=(TOP, TOP))


def test_groups_with_an_empty_one_and_a_nearer_ring_of_a_later_group(dev):
    strokes = [SC.square(100, 100, 20), SC.line(500, 500, 520, 500), SC.square(10, 10, 5), SC.ring(510, 520, 30, 9), SC.line(15, 15, 16, 16), SC.square(400, 400, 50)]
    grp = np.array([0, 0, 2, 2, 2, 0], np.int32)                                                  # group 1 is empty; (10, 10) of group 2 is the nearest to the start
    order, rev, seam, st = same(dev, strokes, grp, 3, (12, 12))
    assert grp[order].tolist() == [0, 0, 0, 2, 2, 2] and order[0] == 0
    same(dev, strokes, grp + 61, 64, (12, 12))                                                    # groups 61 and 63 of 64


def test_medium_case_against_the_double(dev):
    """about 3000 strokes: rings of 5 - 40 vertices among open strokes and dots, in 4 groups"""
    rng = np.random.default_rng(21)
    n = 3000
    c = rng.integers(100, 20000, (n, 2)); m = rng.integers(5, 41, n); t = rng.uniform(0, 6, n); kind = rng.integers(0, 10, n)
    strokes = []
    for i in range(n):
        x, y = int(c[i, 0]), int(c[i, 1])
        strokes.append(SC.ring(x, y, 60, int(m[i]), float(t[i])) if kind[i] < 6 else rng.integers(0, 20000, (int(rng.integers(2, 6)), 2)) if kind[i] < 9 else np.array([[x, y]]))
    grp = rng.integers(0, 4, n).astype(np.int32)
    off, pts, _, _, _ = SC.pack(strokes)
    got = dev.gcode_order_rings(off, pts, grp, 4, True, (10000, 0))
    want = RD.order_rings(off, pts, grp, 4, True, (10000, 0))
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3] and got[3]["closed"] > 1500 and got[3]["moved"] > 1000


# ------------------------------------------------------------------ the device's own plain orders
def test_without_a_ring_it_is_the_plain_orders(dev):
    rng = np.random.default_rng(8)
    n = 5000
    strokes = [rng.integers(0, 3000, (int(rng.integers(2, 5)), 2)) for _ in range(n)]
    for i in range(0, n, 50):
        strokes[i] = np.array([strokes[i][0], strokes[i][1], strokes[i][0]])                      # A, B, A
    off, pts, _, _, _ = SC.pack(strokes)
    ends = np.concatenate([pts[off[:-1]], pts[off[1:] - 1]], 1)
    grp = rng.integers(0, 5, n).astype(np.int32)
    for reverse in (False, True):
        order, rev, seam, st = dev.gcode_order_rings(off, pts, grp, 5, reverse, (1500, 40))
        w_order, w_rev = dev.gcode_order_pens(ends, grp, 5, reverse, (1500, 40))
        assert np.array_equal(order, w_order) and np.array_equal(rev, w_rev) and not seam.any() and st["closed"] == st["moved"] == 0 and st["candidates"] == n * (1 + reverse)
    order, rev, seam, st = dev.gcode_order_rings(off, pts, None, 1)
    assert np.array_equal(order, dev.gcode_order(ends)) and not rev.any()
    from orip import gcode as GC
    assert st["travel"] == GC.travel_steps(*GC.gather_paths(off, pts, order))


# ------------------------------------------------------------------ invariants on a plot too large for the double
def test_ten_thousand_circles(dev):
    from orip import gcode as GC
    rng = np.random.default_rng(9)
    n, m = 10000, 64
    a = 2.0 * np.pi * np.arange(m) / m
    c = rng.integers(200, 29000, (n, 2)); t = rng.uniform(0, 6, n)
    ring = np.stack([np.rint(c[:, None, 0] + 150 * np.cos(a[None, :] + t[:, None])), np.rint(c[:, None, 1] + 150 * np.sin(a[None, :] + t[:, None]))], 2).astype(np.int32)
    pts = np.concatenate([ring, ring[:, :1]], 1).reshape(-1, 2)
    off = np.arange(n + 1, dtype=np.int64) * (m + 1)
    grp = (np.arange(n) % 3).astype(np.int32)
    order, rev, seam, st = dev.gcode_order_rings(off, pts, grp, 3, True, (0, 0))
    assert np.array_equal(np.sort(order), np.arange(n)) and (np.diff(grp[order]) >= 0).all() and not rev.any() and seam.min() >= 0 and seam.max() < m
    assert st["closed"] == n and st["candidates"] == n * m and st["moved"] == int((seam != 0).sum()) > n // 2
    assert st["travel"] == GC.travel_steps(*GC.gather_paths(off, pts, order, rev, seam))
    # the resident form: the strokes the upload of a conversion leaves, read and not changed
    mm_off, mm_pts = off, pts.astype(np.float64)
    s_off, s_pts = dev.gcode_to_steps(mm_off, mm_pts, MAP)
    assert np.array_equal(s_off, off) and np.array_equal(s_pts, pts)
    again = dev.gcode_order_rings(None, None, grp, 3, True, (0, 0))
    assert all(np.array_equal(x, y) for x, y in zip(again[:3], (order, rev, seam))) and again[3] == st
    r_off, r_pts = dev.gcode_steps_fetch(n, len(pts))
    assert np.array_equal(r_off, off) and np.array_equal(r_pts, pts)
    one = dev.gcode_order_rings(off[:3], pts[:off[2]], None, 1)                                    # an explicit input does not become the resident list
    assert len(one[0]) == 2 and np.array_equal(dev.gcode_steps_fetch(n, len(pts))[1], pts)


# ------------------------------------------------------------------ bad arguments
def raw(dev, off, pts, group, n, n_groups, flags, start, outs=(True, True, True, True)):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((off, np.int64), (pts, np.int32), (group, np.int32), (start, np.int32))]
    k = max(int(n), 1) if 0 <= n < 100 else 1
    o_order = np.full(k, -7, np.int32); o_rev = np.full(k, 7, np.uint8); o_seam = np.full(k, -7, np.int32); o_st = np.full(4, -7, np.int64)
    given = [p(a) if on else None for a, on in zip((o_order, o_rev, o_seam, o_st), outs)]
    rc = dev.L.orip_gcode_order_rings(dev.h, p(keep[0]), p(keep[1]), p(keep[2]), int(n), int(n_groups), int(flags), p(keep[3]), *given)
    assert rc == 0 or ((o_order == -7).all() and (o_rev == 7).all() and (o_seam == -7).all() and (o_st == -7).all())      # a refused call touches nothing
    return rc, (dev.L.orip_last_error(dev.h) or b"").decode()


def test_bad_arguments(dev):
    from orip.device import OripError
    off = np.array([0, 5, 7, 12, 13]); pts = np.concatenate([SC.square(0, 0, 9), SC.line(20, 20, 30, 30), SC.square(40, 0, 9), [[3, 3]]])
    g = np.array([0, 1, 1, 0]); s = np.array([0, 0])
    good = (off, pts, g, 4, 2, 1, s)

    def with_pt(i, j, v):
        q = pts.copy(); q[i, j] = v
        return q

    def check_good():
        assert raw(dev, *good)[0] == 0
        got, want = dev.gcode_order_rings(off, pts, g, 2, True), RD.order_rings(off, pts, g, 2, True)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]
    check_good()
    bad = [("n < 0", (off, pts, g, -1, 2, 1, s)), ("n > 2^26", (off, pts, g, (1 << 26) + 1, 2, 1, s)), ("off not from 0", (off + 1, pts, g, 4, 2, 1, s)),
           ("a stroke without a point", (np.array([0, 5, 5, 12, 13]), pts, g, 4, 2, 1, s)), ("offsets decrease", (np.array([0, 7, 5, 12, 13]), pts, g, 4, 2, 1, s)),
           ("off without pts", (off, None, g, 4, 2, 1, s)), ("pts without off", (None, pts, g, 4, 2, 1, s)),
           ("x < 0", (off, with_pt(1, 0, -1), g, 4, 2, 1, s)), ("y > 2^30", (off, with_pt(6, 1, TOP + 1), g, 4, 2, 1, s)),
           ("start < 0", (off, pts, g, 4, 2, 1, np.array([-1, 0]))), ("start > 2^30", (off, pts, g, 4, 2, 1, np.array([0, TOP + 1]))),
           ("a group of 2 of 2", (off, pts, np.array([0, 2, 1, 0]), 4, 2, 1, s)), ("a negative group", (off, pts, np.array([0, -1, 1, 0]), 4, 2, 1, s)),
           ("no groups", (off, pts, g, 4, 0, 1, s)), ("65 groups", (off, pts, g, 4, 65, 1, s)), ("an unknown flag", (off, pts, g, 4, 2, 2, s)),
           ("2^28 points", (np.array([0, 1 << 28]), pts, None, 1, 1, 0, s))]
    for what, args in bad:
        rc, msg = raw(dev, *args)
        assert rc != 0 and "orip_gcode_order_rings" in msg, what
        check_good()
    for i in range(4):                                                                            # a NULL output with n > 0; NULL stats
        rc, msg = raw(dev, *good, outs=tuple(j != i for j in range(4)))
        assert rc != 0 and "orip_gcode_order_rings" in msg
        check_good()
    assert raw(dev, off, pts, g, 0, 2, 1, s, outs=(False, False, False, True))[0] == 0            # n == 0 needs no output but the stats
    assert raw(dev, off, pts, g, 0, 2, 1, s, outs=(False, False, False, False))[0] != 0
    got_off, _ = dev.gcode_to_steps(np.array([0, 2, 4]), np.array([[0.0, 0.0], [5.0, 1.0], [2.0, 2.0], [3.0, 3.0]]), MAP)
    assert len(got_off) == 3
    rc, msg = raw(dev, None, None, g, 4, 2, 1, s)                                                 # four asked for, two resident
    assert rc != 0 and "resident" in msg
    check_good()
    assert np.array_equal(dev.gcode_steps_fetch(2, 4)[0], got_off)                                # the resident list is what it was
    assert raw(dev, None, None, None, 2, 1, 0, None)[0] == 0
    for call in (lambda: dev.gcode_order_rings(off, pts, [0, 1, 1], 2), lambda: dev.gcode_order_rings(off, pts, g, 2, start=(-1, 0)),
                 lambda: dev.gcode_order_rings(off, None, g, 2), lambda: dev.gcode_order_rings(None, None, g, 2), lambda: dev.gcode_order_rings(None, None, None, 1)):
        with pytest.raises((OripError, ValueError)):
            call()
    check_good()


# ------------------------------------------------------------------ the whole tools
GCODE_DOUBLES = dict(steps_fn=D.to_steps_numpy, order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)
SEAM = dict(seam_fn=lambda off, pts, order, rev: SD.seams(off, pts, order, rev, (0, 0)))
IMPROVE = dict(improve_fn=lambda ends, group, n_groups, order, rev, reverse, max_rounds: ID.improve(ends, group, n_groups, order, rev, reverse, (0, 0), max_rounds))
RINGS = dict(ring_entry_fn=RD.order_rings_fn)


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


def decode(dev, data, info):
    from orip import stream_preview as SP
    W, H = info["target"]
    return SP.preview(dev, data, W, H, 320, 240, invert_y=True)[1]


def run(script, args):
    return subprocess.run([sys.executable, os.path.join(SCRIPTS, script)] + args, capture_output=True, text=True, timeout=300)


def last_travel(info):
    return info["seam"]["travel_after"] if "seam" in info else info["improve"]["travel_after"] if "improve" in info else info["ring_entry"]["travel"]


def decoded_as_the_rule_says(dev, got, info, plain, pinfo, plain_travel):
    """the stream differs from the plain order's by its pen-up steps alone, and they are what the passes report"""
    st, pst = decode(dev, got, info), decode(dev, plain, pinfo)
    assert st["steps_total"] == info["steps"] == pst["steps_total"] - plain_travel + last_travel(info)
    assert st["pen_down_segments"] == pst["pen_down_segments"] and st["color_changes"] == pst["color_changes"] and st["eof_seen"] == 1 and st["off_canvas_draws"] == 0


def test_svg_tool(dev, tmp_path):
    from orip import svg as SV, gcode as GC
    src = tmp_path / "drawing.svg"
    src.write_bytes(SC.TOOL_SVG)
    for extra, dbl in (([], lambda: dict(__import__("svg_double").svg_doubles(), **RINGS)),
                       (SC.TOOL_SVG_ARGS + ["--improve-order", "--loop-start"], lambda: dict(PD.pens_doubles(), **IMPROVE, **SEAM, **RINGS))):
        args = extra + ["--ring-entry"]
        want, winfo = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(args), **dbl())
        got, info = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(args), dev)
        assert got == want and info["ring_entry"] == winfo["ring_entry"] and info["ring_entry"]["closed"] == 12 and info.get("pens") == winfo.get("pens")
        assert info.get("seam") == winfo.get("seam") and info.get("improve") == winfo.get("improve")
        plain, pinfo = SV.build_stream_from_svg(SC.TOOL_SVG, svg_options(extra + ["--loop-start"] if not extra else extra), dev)
        assert "ring_entry" not in pinfo
        decoded_as_the_rule_says(dev, got, info, plain, pinfo, pinfo["seam"]["travel_after"])
        r = run("svg2stream.py", [str(src), "--no-preview"] + args)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert (tmp_path / "drawing_stream.bin").read_bytes() == want and GC.ring_entry_line("svg", info["ring_entry"]) in r.stdout
        gcode_with = (tmp_path / "drawing.gcode").read_text()
        r = run("svg2stream.py", [str(src), "--no-preview"] + extra)
        assert r.returncode == 0 and (tmp_path / "drawing.gcode").read_text() == gcode_with and "ring entry" not in r.stdout      # the G-code file is unchanged
    assert run("svg2gcode.py", [str(src), "-o", str(tmp_path / "x.gcode"), "--ring-entry"]).returncode != 0      # svg2gcode.py does not get the option
    assert run("svg2stream.py", [str(src), "--no-preview", "--ring-entry", "--no-reorder"]).returncode != 0


def test_gcode_tool(dev, tmp_path):
    from orip import gcode as GC
    text = SC.tool_gcode()
    S = PD.StepsWithSource()
    for kw in (dict(), dict(loop_start=True), dict(improve_order=True, loop_start=True, allow_reverse=True), dict(merge_paths=True, simplify_mm=0.0, loop_start=True)):
        dbl = dict(GCODE_DOUBLES, **IMPROVE, **SEAM, **RINGS)
        if "allow_reverse" in kw:
            dbl = dict(dbl, steps_fn=S.steps, source_fn=S.source, order_pens_fn=PD.order_pens_numpy)
        if "merge_paths" in kw:
            import merge_double as MD
            import simplify_double as SPD
            dbl = dict(dbl, merge_fn=MD.merge_numpy, simplify_fn=SPD.simplify_numpy)
        want, winfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(ring_entry=True, **kw), **dbl)
        got, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(ring_entry=True, **kw), dev)
        assert got == want and info["ring_entry"] == winfo["ring_entry"] and info["ring_entry"]["closed"] == 20, kw
        assert info.get("seam") == winfo.get("seam") and info.get("improve") == winfo.get("improve")
        pkw = dict(kw, loop_start=True)                                                           # the plain order, whose travel the seam pass reports
        plain, pinfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(**pkw), dev)
        assert "ring_entry" not in pinfo
        decoded_as_the_rule_says(dev, got, info, plain, pinfo, pinfo["seam"]["travel_after"])
    (tmp_path / "drawing.gcode").write_text(text)
    for flags, kw in ((["--ring-entry"], dict()), (["--ring-entry", "--improve-order", "--loop-start", "--allow-reverse"], dict(improve_order=True, loop_start=True, allow_reverse=True))):
        dbl = dict(GCODE_DOUBLES, **IMPROVE, **SEAM, **RINGS)
        if kw:
            dbl = dict(dbl, steps_fn=S.steps, source_fn=S.source, order_pens_fn=PD.order_pens_numpy)
        want, winfo = GC.build_stream_from_gcode(text, GC.GcodeOptions(ring_entry=True, **kw), **dbl)
        r = run("gcode2stream.py", [str(tmp_path / "drawing.gcode"), "-o", str(tmp_path / "out.bin")] + flags)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert (tmp_path / "out.bin").read_bytes() == want and GC.ring_entry_line("gcode", winfo["ring_entry"]) in r.stdout
    r = run("gcode2stream.py", [str(tmp_path / "drawing.gcode"), "-o", str(tmp_path / "no.bin"), "--ring-entry", "--no-reorder"])
    assert r.returncode != 0 and not (tmp_path / "no.bin").exists()


def test_tool_unchanged_without_the_option(dev):
    from orip import svg as SV, gcode as GC
    got, info = SV.build_stream_from_svg(PD.TOOL_SVG, svg_options(PD.TOOL_PLAIN_ARGS), dev)
    assert got == bytes(GP["tool_plain_stream"]) and "ring_entry" not in info
    text = SC.tool_gcode()
    want, _ = GC.build_stream_from_gcode(text, GC.GcodeOptions(loop_start=True), **dict(GCODE_DOUBLES, **SEAM, ring_entry_fn=None))
    got, info = GC.build_stream_from_gcode(text, GC.GcodeOptions(loop_start=True), dev)
    assert got == want and "ring_entry" not in info
