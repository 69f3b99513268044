"""TEST INFRASTRUCTURE: --clip as include/orip.h states it (orip_gcode_to_steps_clip), one path at a time and one segment at a time, in Python integers and
fractions.Fraction: the parameter interval of a segment inside the rectangle as exact rationals, the cut points rounded from the exact point, the strokes
put together by walking the segments in order.  Written as the definition, not the fast way, and independently of csrc/gcode_clip.hip (no candidates, no
scans).  The conversion is gcode_double.to_steps_numpy's arithmetic without its clamp."""
import math
from fractions import Fraction

import numpy as np

TOP = 1 << 30
STATS = ("segments", "inside", "cut", "outside", "paths_out", "points_out")


class RangeError(ValueError):
    """a rounded coordinate outside [-2^30, 2^30]: the drawing is that far off the sheet"""


def unclamped_steps(pts_mm, m):
    """the rounded step coordinates of every point as float64 (x, y); what to_steps_numpy computes before it clamps"""
    p = np.asarray(pts_mm, np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        x = (p[:, 0] * m["scale_x"] + m["offset_x_mm"]) * m["steps_per_mm"]
        y = (p[:, 1] * m["scale_y"] + m["offset_y_mm"]) * m["steps_per_mm"]
        if m["invert_y"]:
            y = float(m["H"] - 1) - y
        x, y = np.rint(x), np.rint(y)
    return x, y


def sheet(m, margin=0):
    return margin, margin, m["W"] - 1 - margin, m["H"] - 1 - margin


def interval(v0, v1, rect):
    """the t in [0, 1] with v0 + t (v1 - v0) inside the closed rectangle: (t0, t1) as Fractions, or None"""
    x0, y0, x1, y1 = rect
    t0, t1 = Fraction(0), Fraction(1)
    for v, w, lo, hi in ((v0[0], v1[0], x0, x1), (v0[1], v1[1], y0, y1)):
        d = w - v
        if d == 0:
            if not (lo <= v <= hi):
                return None
            continue
        a, b = Fraction(lo - v, d), Fraction(hi - v, d)            # where the line meets the two sides
        t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
    return (t0, t1) if t0 <= t1 else None


def point_at(v0, v1, t):
    """the exact point, each coordinate to the nearest step, halves toward +infinity"""
    return tuple(math.floor(v0[k] + t * (v1[k] - v0[k]) + Fraction(1, 2)) for k in (0, 1))


def clip_path(v, rect):
    """the strokes of one path of integer points, and (inside, cut, outside)"""
    strokes, cur = [], None
    inside = cut = outside = 0
    open_end = False                                               # the segment before ended with t1 = 1, non-empty
    for a, b in zip(v[:-1], v[1:]):
        iv = interval(a, b, rect)
        if iv is None:
            outside += 1; open_end = False
            continue
        t0, t1 = iv
        if t0 == 0 and t1 == 1: inside += 1
        else: cut += 1
        if not (open_end and t0 == 0):
            cur = [point_at(a, b, t0)]; strokes.append(cur)
        B = point_at(a, b, t1)
        if B != cur[-1]:
            cur.append(B)
        open_end = t1 == 1
    return [s for s in strokes if len(s) >= 2], (inside, cut, outside)


def clip_numpy(off, pts_mm, m, rect):
    """-> (off int64, pts int32 [total, 2], src int32, stats dict)"""
    off = np.asarray(off, np.int64).reshape(-1)
    x, y = unclamped_steps(pts_mm, m)
    out, src = [], []
    tot = [0, 0, 0]
    for p in range(max(len(off) - 1, 0)):
        a, b = int(off[p]), int(off[p + 1])
        if b - a < 2:
            continue
        if not (np.isfinite(x[a:b]) & np.isfinite(y[a:b])).all():
            raise OverflowError("a coordinate is not finite after the conversion to steps")
        v = [(int(xx), int(yy)) for xx, yy in zip(x[a:b].tolist(), y[a:b].tolist())]
        if any(abs(c) > TOP for q in v for c in q):
            raise RangeError("a point lies more than 2^30 steps off the sheet")
        strokes, counts = clip_path(v, tuple(int(r) for r in rect))
        out += strokes; src += [p] * len(strokes)
        tot = [s + c for s, c in zip(tot, counts)]
    lens = [len(s) for s in out]
    pts = np.asarray([q for s in out for q in s], np.int32).reshape(-1, 2)
    st = dict(zip(STATS, (sum(tot), *tot, len(out), len(pts))))
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), pts, np.asarray(src, np.int32), st


class ClipWithSource:
    """clip_numpy as the clip_fn of orip.gcode.build_stream_from_gcode, with the sources kept for source_fn"""
    def __init__(self): self.src = np.zeros(0, np.int32); self.calls = []

    def clip(self, off, pts_mm, m, rect):
        o, p, self.src, st = clip_numpy(off, pts_mm, m, rect)
        self.calls.append((tuple(rect), st))
        return o, p, st

    def clip_paths(self, paths, m, rect):                          # the form of orip.svg.build_stream_from_svg
        return self.clip(paths[0], paths[1], m, rect)

    def source(self, n):
        assert n == len(self.src)
        return self.src


def gcode_doubles():
    """the keyword arguments that put every device step of orip.gcode.build_stream_from_gcode on the CPU, --clip and the options it works with included"""
    import gcode_double as D
    import merge_double as MD
    import improve_double as ID
    import pens_double as PD
    from stream_double import codes_numpy
    S, K = PD.StepsWithSource(), ClipWithSource()
    return dict(steps_fn=S.steps, clip_fn=K.clip, source_fn=lambda n: K.source(n) if K.calls else S.source(n), order_fn=D.order_numpy, order_pens_fn=PD.order_pens_numpy,
                merge_fn=MD.merge_numpy, improve_fn=lambda ends, group, n_groups, order, rev, reverse, max_rounds: ID.improve(ends, group, n_groups, order, rev, reverse, (0, 0), max_rounds),
                codes_fn=codes_numpy, pack_fn=D.pack_numpy)


def svg_doubles():
    """the same for orip.svg.build_stream_from_svg"""
    import pens_double as PD
    g = gcode_doubles()
    K = ClipWithSource()
    base = PD.pens_doubles()
    return dict(base, clip_fn=K.clip_paths, source_fn=lambda n: K.source(n) if K.calls else base["source_fn"](n), merge_fn=g["merge_fn"], improve_fn=g["improve_fn"])
