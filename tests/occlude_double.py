"""A sequential double of --occlude (include/orip.h: orip_gcode_occlude), written from the rule and sharing nothing with the device code: Python integers
and Fractions.  Per segment it collects every parameter at which something can change (where the segment's line meets an edge, where a collinear edge
begins and ends), tests the MIDPOINT of every elementary interval with an exact on-edge test and an exact even-odd ray test against every shape above
the stroke, joins the visible intervals into pieces and rounds their ends.  occlude_numpy has the signature and the result of Device.gcode_occlude;
rings_to_steps is the ring conversion of Device.svg_occlude through tests/gcode_double.py's arithmetic."""
from fractions import Fraction

import numpy as np

TOP = 1 << 30
STATS = ("segments", "whole", "cut", "hidden", "pieces", "collapsed", "paths_out", "points_out", "draw_steps_in", "draw_steps_out")


def _check(off, pts, level, ring_off, ring_pts, ring_level):
    n, m = len(off) - 1, len(ring_off) - 1
    if n < 0 or m < 0 or len(level) != n or len(ring_level) != m:
        raise ValueError("counts")
    if off[0] != 0 or ring_off[0] != 0:
        raise ValueError("offsets must start at 0")
    for p in range(n):
        if off[p + 1] - off[p] < 2:
            raise ValueError(f"stroke {p} has fewer than two points")
        if not 0 <= level[p] < TOP:
            raise ValueError(f"stroke {p}: level")
    for r in range(m):
        if ring_off[r + 1] - ring_off[r] < 1:
            raise ValueError(f"ring {r} has no points")
        if not 0 <= ring_level[r] < TOP:
            raise ValueError(f"ring {r}: level")
        if r and ring_level[r] < ring_level[r - 1]:
            raise ValueError("ring_level must not decrease")
    if len(pts) != off[-1] or len(ring_pts) != ring_off[-1]:
        raise ValueError("points")
    for x, y in pts:
        if not (0 <= x <= TOP and 0 <= y <= TOP):
            raise ValueError("stroke coordinate outside 0..2^30")
    for x, y in ring_pts:
        if not (-TOP <= x <= TOP and -TOP <= y <= TOP):
            raise ValueError("ring coordinate outside +-2^30")
    for p in range(n):
        for i in range(off[p] + 1, off[p + 1]):
            if pts[i] == pts[i - 1]:
                raise ValueError(f"stroke {p}: a point equals the one before it")


def _shapes(ring_off, ring_pts, ring_level):
    """[(level, edges, box)] in ascending level; an edge is ((px, py), (qx, qy)) of positive length"""
    by = {}
    for r in range(len(ring_off) - 1):
        ring = ring_pts[ring_off[r]:ring_off[r + 1]]
        e = by.setdefault(ring_level[r], ([], []))
        e[1].extend(ring)
        for k, P in enumerate(ring):
            Q = ring[(k + 1) % len(ring)]
            if P != Q:
                e[0].append((P, Q))
    out = []
    for lv in sorted(by):
        edges, allp = by[lv]
        xs = [p[0] for p in allp]; ys = [p[1] for p in allp]
        out.append((lv, edges, (min(xs), min(ys), max(xs), max(ys))))
    return out


def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def _inside(edges, x, y):
    """the rational point strictly inside the even-odd region of the edges: on no edge, and a ray toward +x crosses an odd number"""
    odd = False
    for (px, py), (qx, qy) in edges:
        if _cross(qx - px, qy - py, x - px, y - py) == 0 and min(px, qx) <= x <= max(px, qx) and min(py, qy) <= y <= max(py, qy):
            return False
        if (py > y) != (qy > y):
            xi = px + Fraction((y - py) * (qx - px), qy - py)
            if xi > x:
                odd = not odd
    return odd


def _round(v):
    """nearest integer, halves toward +infinity"""
    return (2 * v.numerator + v.denominator) // (2 * v.denominator)


def segment_pieces(A, B, shapes):
    """the pieces [(t0, t1)] of A -> B under the shapes (each (level, edges, box)), as Fractions in order"""
    ax, ay = A; dx, dy = B[0] - ax, B[1] - ay
    box = (min(ax, B[0]), min(ay, B[1]), max(ax, B[0]), max(ay, B[1]))
    near = [s for s in shapes if s[2][0] <= box[2] and s[2][2] >= box[0] and s[2][1] <= box[3] and s[2][3] >= box[1]]
    ts = {Fraction(0), Fraction(1)}
    L = dx * dx + dy * dy
    for _, edges, _ in near:
        for (px, py), (qx, qy) in edges:
            ex, ey = qx - px, qy - py
            den = _cross(ex, ey, dx, dy)
            if den == 0:
                if _cross(dx, dy, px - ax, py - ay) == 0:                        # collinear: where the edge begins and ends
                    for x, y in ((px, py), (qx, qy)):
                        ts.add(Fraction((x - ax) * dx + (y - ay) * dy, L))
                continue
            t = Fraction(_cross(ex, ey, px - ax, py - ay), den)                   # where the two LINES meet ...
            u = Fraction(_cross(dx, dy, px - ax, py - ay), den)                   # ... and where on the edge's: P + u e
            if 0 <= u <= 1:
                ts.add(t)
    ts = sorted(t for t in ts if 0 <= t <= 1)
    pieces = []
    for a, b in zip(ts[:-1], ts[1:]):
        mid = (a + b) / 2
        x, y = ax + mid * dx, ay + mid * dy
        if any(_inside(edges, x, y) for _, edges, _ in near):
            continue
        if pieces and pieces[-1][1] == a:
            pieces[-1] = (pieces[-1][0], b)
        else:
            pieces.append((a, b))
    return pieces


def occlude_lists(strokes, levels, rings, ring_levels):
    """strokes / rings as lists of lists of (x, y) -> (out strokes as lists of (x, y), origin, stats dict)"""
    by = _shapes(np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(int).tolist(), [tuple(p) for r in rings for p in r], list(ring_levels))
    out, origin = [], []
    st = dict.fromkeys(STATS, 0)
    for k, stroke in enumerate(strokes):
        above = [s for s in by if s[0] > levels[k]]
        cur = None                                                                # the open output stroke; it can go on only through a vertex
        for j in range(len(stroke) - 1):
            A, B = tuple(stroke[j]), tuple(stroke[j + 1])
            st["segments"] += 1
            st["draw_steps_in"] += max(abs(B[0] - A[0]), abs(B[1] - A[1]))
            pieces = segment_pieces(A, B, above) if above else [(Fraction(0), Fraction(1))]
            st["pieces"] += len(pieces)
            st["whole" if pieces == [(0, 1)] else "cut" if pieces else "hidden"] += 1
            reaches = None                                                        # the stroke that goes on through B
            for q, (t0, t1) in enumerate(pieces):
                P = A if t0 == 0 else (_round(A[0] + t0 * (B[0] - A[0])), _round(A[1] + t0 * (B[1] - A[1])))
                Q = B if t1 == 1 else (_round(A[0] + t1 * (B[0] - A[0])), _round(A[1] + t1 * (B[1] - A[1])))
                if P == Q:
                    st["collapsed"] += 1
                    continue
                st["draw_steps_out"] += max(abs(Q[0] - P[0]), abs(Q[1] - P[1]))
                if q == 0 and t0 == 0 and cur is not None:
                    cur.append(Q); into = cur
                else:
                    into = [P, Q]; out.append(into); origin.append(k)
                if q == len(pieces) - 1 and t1 == 1:
                    reaches = into
            cur = reaches
    st["paths_out"] = len(out); st["points_out"] = sum(len(s) for s in out)
    return out, origin, st


def occlude_numpy(off, pts, level, ring_off, ring_pts, ring_level, n=None):
    """Device.gcode_occlude: (off int64, pts int32 [total', 2], origin int32 [paths_out], {STATS})"""
    off = [int(v) for v in np.asarray(off).reshape(-1)]; ring_off = [int(v) for v in np.asarray(ring_off).reshape(-1)]
    pts = [(int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2)]; ring_pts = [(int(x), int(y)) for x, y in np.asarray(ring_pts).reshape(-1, 2)]
    level = [int(v) for v in np.asarray(level).reshape(-1)]; ring_level = [int(v) for v in np.asarray(ring_level).reshape(-1)]
    _check(off, pts, level, ring_off, ring_pts, ring_level)
    strokes = [pts[a:b] for a, b in zip(off[:-1], off[1:])]
    rings = [ring_pts[a:b] for a, b in zip(ring_off[:-1], ring_off[1:])]
    out, origin, st = occlude_lists(strokes, level, rings, ring_level)
    o = np.concatenate([[0], np.cumsum([len(s) for s in out])]).astype(np.int64)
    p = np.asarray([q for s in out for q in s], np.int32).reshape(-1, 2)
    return o, p, np.asarray(origin, np.int32), st


def rings_to_steps(paths_off, paths_mm, ring_sub, map_, clamp):
    """the rings of Device.svg_occlude: fitted path ring_sub[r], every point converted as the conversion converts it (tests/gcode_double.py), clamped to
    the sheet or not, no point dropped -> (ring_off int64, ring_pts int32 [R, 2])"""
    off, pts = [0], []
    for r in ring_sub:
        mm = np.asarray(paths_mm[paths_off[r]:paths_off[r + 1]], np.float64).reshape(-1, 2)
        x = (mm[:, 0] * map_["scale_x"] + map_["offset_x_mm"]) * map_["steps_per_mm"]      # gcode_double.to_steps_numpy's arithmetic, point for point
        y = (mm[:, 1] * map_["scale_y"] + map_["offset_y_mm"]) * map_["steps_per_mm"]
        if map_["invert_y"]:
            y = float(map_["H"] - 1) - y
        xy = np.stack([np.rint(x), np.rint(y)], 1).astype(np.int64)
        if clamp:
            xy = np.stack([np.clip(xy[:, 0], 0, map_["W"] - 1), np.clip(xy[:, 1], 0, map_["H"] - 1)], 1)
        pts.extend(xy.tolist()); off.append(len(pts))
    return np.asarray(off, np.int64), np.asarray(pts, np.int64).reshape(-1, 2).astype(np.int32)
