"""The sequential double of --dedup (include/orip.h: orip_gcode_dedup), in plain Python integers, written from the rule and not from the kernel: segment
after segment in drawing order, every line's union of earlier intervals kept as a sorted list of disjoint closed intervals, the survivors of a segment read
off it.  No numpy arithmetic touches a coordinate; numpy only carries the arrays in and out.  primitive_steps() expands a drawing into its lattice steps,
the multiset the first consequence of the rule is stated on."""
from bisect import bisect_left, bisect_right
from math import gcd

import numpy as np

TOP = 1 << 30
STATS = ("segments", "whole", "cut", "covered", "pieces", "paths_out", "points_out", "draw_steps_in", "draw_steps_out")


def line_of(group, a, b):
    """(LINE, tau(a), tau(b)) of the segment a -> b; LINE = (group, ux, uy, c)"""
    dx, dy = b[0] - a[0], b[1] - a[1]
    q = gcd(abs(dx), abs(dy))
    ux, uy = dx // q, dy // q
    if ux < 0 or (ux == 0 and uy < 0):
        ux, uy = -ux, -uy
    c = ux * a[1] - uy * a[0]
    assert c == ux * b[1] - uy * b[0] and abs(c) <= 1 << 61
    t = 0 if ux > 0 else 1
    return (group, ux, uy, c), a[t], b[t]


def pieces_of(lo, hi, los, his):
    """the components of positive length of the closure of [lo, hi] minus the union (los[i], his[i]: disjoint closed intervals, ascending), ascending"""
    out, cover = [], lo
    i = bisect_right(his, lo)                             # the first interval that reaches beyond lo
    while i < len(los) and los[i] < hi:
        if los[i] > cover:
            out.append((cover, los[i]))
        cover = his[i]
        i += 1
    if cover < hi:
        out.append((cover, hi))
    return out


def add_interval(lo, hi, los, his):
    """the union with [lo, hi]: closed intervals that overlap or touch become one"""
    i0, i1 = bisect_left(his, lo), bisect_right(los, hi)
    if i0 < i1:
        lo, hi = min(lo, los[i0]), max(hi, his[i1 - 1])
    los[i0:i1] = [lo]; his[i0:i1] = [hi]


def dedup_lists(strokes, groups=None):
    """strokes: lists of (x, y); groups: one per stroke or None.  -> (output strokes, origin, stats dict)"""
    groups = [0] * len(strokes) if groups is None else [int(g) for g in groups]
    lines = {}                                            # LINE -> (los, his: the union of the segments so far, {tau: point} of every end on it)
    out, origin = [], []
    st = dict.fromkeys(STATS, 0)
    for s, pts in enumerate(strokes):
        pts = [(int(x), int(y)) for x, y in pts]
        cur = None                                        # the open output stroke: the segment before still reaches the vertex it shares with the next
        for a, b in zip(pts[:-1], pts[1:]):
            key, ta, tb = line_of(groups[s], a, b)
            los, his, at = lines.setdefault(key, ([], [], {}))
            lo, hi = min(ta, tb), max(ta, tb)
            at.setdefault(ta, a); at.setdefault(tb, b)
            assert at[ta] == a and at[tb] == b
            ps = [(at[l], at[h]) for l, h in pieces_of(lo, hi, los, his)]
            if tb < ta:
                ps = [(q, p) for p, q in reversed(ps)]
            st["segments"] += 1
            st["draw_steps_in"] += max(abs(b[0] - a[0]), abs(b[1] - a[1]))
            st["whole" if ps == [(a, b)] else "cut" if ps else "covered"] += 1
            for k, (p, q) in enumerate(ps):
                st["pieces"] += 1
                st["draw_steps_out"] += max(abs(q[0] - p[0]), abs(q[1] - p[1]))
                if k == 0 and cur is not None and p == a:
                    cur.append(q)
                else:
                    cur = [p, q]; out.append(cur); origin.append(s)
            if not ps or ps[-1][1] != b:
                cur = None                                # the next segment cannot continue: its first vertex is not reached
            add_interval(lo, hi, los, his)
    st["paths_out"] = len(out); st["points_out"] = sum(len(p) for p in out)
    return out, origin, st


def check_input(off, pts, group, n_groups):
    off = np.asarray(off, np.int64).reshape(-1); pts = np.asarray(pts, np.int64).reshape(-1, 2)
    n = len(off) - 1
    if n < 0 or off[0] != 0 or (np.diff(off) < 2).any() or int(off[-1]) != len(pts):
        raise ValueError("offsets")
    if len(pts) and (pts.min() < 0 or pts.max() > TOP):
        raise ValueError("a coordinate outside 0..2^30")
    if not (1 <= int(n_groups) <= 64):
        raise ValueError("n_groups")
    g = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64).reshape(-1)
    if len(g) != n or (g < 0).any() or (g >= n_groups).any():
        raise ValueError("group")
    same = np.ones(len(pts), bool)
    if len(pts):
        same[1:] = (np.diff(pts, axis=0) == 0).all(1); same[off[:-1]] = False
    if same[:len(pts)].any() and len(pts):
        raise ValueError("a point equals the one before it")
    return off, pts, g


def dedup_numpy(off, pts, group=None, n_groups=1, n=None):
    """what orip.device.Device.gcode_dedup returns: (off int64, pts int32 [total, 2], origin int32, stats dict)"""
    off, pts, g = check_input(off, pts, group, n_groups)
    strokes = [[tuple(q) for q in pts[a:b].tolist()] for a, b in zip(off[:-1].tolist(), off[1:].tolist())]
    out, origin, st = dedup_lists(strokes, g.tolist())
    o = np.concatenate([[0], np.cumsum([len(p) for p in out])]).astype(np.int64)
    p = np.asarray([q for s in out for q in s], np.int32).reshape(-1, 2)
    return o, p, np.asarray(origin, np.int32), st


def primitive_steps(off, pts, group=None):
    """{(group, P, Q): multiplicity} over the unordered pairs of neighbouring grid points of every segment"""
    off = np.asarray(off, np.int64).reshape(-1).tolist(); P = np.asarray(pts, np.int64).reshape(-1, 2).tolist()
    cnt = {}
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        gr = 0 if group is None else int(group[s])
        for (x0, y0), (x1, y1) in zip(P[a:b - 1], P[a + 1:b]):
            q = gcd(abs(x1 - x0), abs(y1 - y0))
            sx, sy = (x1 - x0) // q, (y1 - y0) // q
            for k in range(q):
                u, v = (x0 + k * sx, y0 + k * sy), (x0 + (k + 1) * sx, y0 + (k + 1) * sy)
                key = (gr, min(u, v), max(u, v))
                cnt[key] = cnt.get(key, 0) + 1
    return cnt
