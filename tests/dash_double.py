"""The sequential double of orip_gcode_dash (include/orip.h states the rule): every stroke by itself, every on-interval by itself, in Python integers with
math.isqrt -- the obvious way, no closed form per segment.  dash_numpy(off, pts, pattern, phase, pat_off, pat_val) -> (off int64, pts int32 [total, 2],
origin int32 [paths_out], {DASH_STATS}), the signature of orip.device.Device.gcode_dash and of the dash step of orip.gcode."""
from bisect import bisect_left, bisect_right
from math import isqrt

import numpy as np

U = 256                                             # units per step
DASH_STATS = ("paths_in", "dashed", "dashes", "collapsed", "paths_out", "points_out", "length_in", "length_on")
ENTRY_MIN, ENTRY_MAX, ENTRIES_MAX, LENGTH_MAX = 256, 1 << 40, 64, 1 << 62


def check_table(pat_off, pat_val):
    """the patterns as lists of Python integers; ValueError for what the rule calls an argument error"""
    pat_off = [int(v) for v in np.asarray(pat_off).reshape(-1)]; pat_val = [int(v) for v in np.asarray(pat_val).reshape(-1)]
    if not pat_off or pat_off[0] != 0 or len(pat_off) - 1 > (1 << 20):
        raise ValueError("pat_off must start at 0 and name 0 .. 2^20 patterns")
    pats = []
    for a, b in zip(pat_off[:-1], pat_off[1:]):
        m = b - a
        if m < 2 or m > ENTRIES_MAX or m % 2 or b > len(pat_val):
            raise ValueError(f"a pattern of {m} entries")
        if any(not (ENTRY_MIN <= e <= ENTRY_MAX) for e in pat_val[a:b]):
            raise ValueError("an entry outside 256 .. 2^40")
        pats.append(pat_val[a:b])
    return pats


def lengths(v):
    """S_0 .. S_end of the stroke v (a list of points): floor(256 sqrt(D)) per segment, summed"""
    S = [0]
    for (x0, y0), (x1, y1) in zip(v[:-1], v[1:]):
        D = (x1 - x0) ** 2 + (y1 - y0) ** 2
        if D == 0:
            raise ValueError("a point equal to the one before it")
        S.append(S[-1] + isqrt(65536 * D))
    return S


def cut_point(v, S, s):
    """the point at arc position s: the vertex itself where s = S_j, else the exact point of its segment rounded to the nearest step, halves toward +infinity"""
    j = bisect_right(S, s) - 1
    if S[j] == s:
        return v[j]
    l, t = S[j + 1] - S[j], s - S[j]
    return tuple(a + (2 * (b - a) * t + l) // (2 * l) for a, b in zip(v[j], v[j + 1]))


def dash_stroke(v, pat, phase):
    """-> (dashes: lists of points, collapsed ones as lists of one point; S_end; on-length)"""
    A = [0]
    for e in pat:
        A.append(A[-1] + e)
    P = A[-1]
    if not (0 <= phase < P):
        raise ValueError("phase outside [0, P)")
    S = lengths(v)
    end = S[-1]
    if end >= LENGTH_MAX:
        raise ValueError("a stroke of 2^62 units or more")
    out, on, r = [], 0, 0
    while r * P - phase < end:
        for i in range(0, len(pat), 2):
            s0, s1 = max(r * P + A[i] - phase, 0), min(r * P + A[i + 1] - phase, end)
            if s1 <= s0:
                continue
            on += s1 - s0
            d = [cut_point(v, S, s0)] + [v[j] for j in range(bisect_right(S, s0), bisect_left(S, s1))] + [cut_point(v, S, s1)]
            out.append([p for k, p in enumerate(d) if k == 0 or p != d[k - 1]])
        r += 1
    return out, end, on


def dash_numpy(off, pts, pattern, phase, pat_off, pat_val):
    off = [int(a) for a in np.asarray(off).reshape(-1)]; pts = np.asarray(pts, np.int64).reshape(-1, 2)
    n = len(off) - 1
    pattern = [int(a) for a in np.asarray(pattern).reshape(-1)]; phase = [int(a) for a in np.asarray(phase).reshape(-1)]
    pats = check_table(pat_off, pat_val)
    if len(pattern) != n or len(phase) != n or any(not (-1 <= p < len(pats)) for p in pattern):
        raise ValueError("one pattern in -1 .. np - 1 and one phase per stroke")
    st = dict.fromkeys(DASH_STATS, 0)
    st["paths_in"] = n
    o_off, o_pts, origin = [0], [], []
    for k in range(n):
        v = [tuple(p) for p in pts[off[k]:off[k + 1]].tolist()]
        if len(v) < 2:
            raise ValueError("a stroke under two points")
        if pattern[k] < 0:
            strokes = [v]
        else:
            strokes, length, on = dash_stroke(v, pats[pattern[k]], phase[k])
            st["dashed"] += 1; st["dashes"] += len(strokes); st["length_in"] += length; st["length_on"] += on
            st["collapsed"] += sum(len(d) < 2 for d in strokes)
            strokes = [d for d in strokes if len(d) >= 2]
        for d in strokes:
            o_pts += d; o_off.append(len(o_pts)); origin.append(k)
    st["paths_out"], st["points_out"] = len(origin), len(o_pts)
    return np.asarray(o_off, np.int64), np.asarray(o_pts, np.int32).reshape(-1, 2), np.asarray(origin, np.int32), st
