"""TEST INFRASTRUCTURE: --hatch-connect restated sequentially (the rule of include/orip.h: orip_gcode_hatch_link), in plain Python integers, over ALL pairs of
lines and all edges of a shape, written from the rule and sharing nothing with csrc/gcode_link.hip: no grid, no sort, no wave, no atomics.  Python integers
do not overflow, so the 128-bit products of the rule are simply products here."""
import numpy as np

STATS = ("lines", "in_reach", "eligible", "links", "coincident", "paths_out", "points_out", "link_steps")
REACH_MAX = 1 << 20


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _on_segment(p, a, b):
    """p lies on the closed segment a b"""
    return _cross(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def segments_meet(e, s, a, b):
    """the closed segments e s and a b share a point; e == s is a segment of one point"""
    if e == s:
        return _on_segment(e, a, b)
    c1, c2, c3, c4 = _cross(a, b, e), _cross(a, b, s), _cross(e, s, a), _cross(e, s, b)
    if ((c1 > 0 > c2) or (c1 < 0 < c2)) and ((c3 > 0 > c4) or (c3 < 0 < c4)):
        return True
    return _on_segment(e, a, b) or _on_segment(s, a, b) or _on_segment(a, e, s) or _on_segment(b, e, s)


def inside(p, edges):
    """even-odd, the boundary is not inside: a ray from p towards +x, an edge taken with its lower end and without its upper one"""
    if any(_on_segment(p, a, b) for a, b in edges):
        return False
    k = 0
    for a, b in edges:
        lo, hi = (a, b) if a[1] < b[1] else (b, a)
        if lo[1] <= p[1] < hi[1] and _cross(lo, hi, p) > 0:      # p lies strictly left of the upward edge: the crossing lies to its right
            k += 1
    return k % 2 == 1


def shape_edges(ring_off, ring_pts, ring_group):
    """{g: the edges of shape g, those of zero length left out}"""
    shapes = {}
    for r, g in enumerate(ring_group):
        ring = [tuple(q) for q in ring_pts[ring_off[r]:ring_off[r + 1]]]
        for a, b in zip(ring, ring[1:] + ring[:1]):
            if a != b:
                shapes.setdefault(int(g), []).append((a, b))
    return shapes


def hatch_link(off, pts, cls, ring_off, ring_pts, ring_group, reach):
    """-> (off int64, pts int32 [total', 2], member_off int64 [paths_out + 1], member int32 [n], {STATS})"""
    off = [int(v) for v in np.asarray(off).reshape(-1)]
    P = [tuple(int(v) for v in q) for q in np.asarray(pts).reshape(-1, 2).tolist()]
    cls = [int(v) for v in np.asarray(cls).reshape(-1)]
    ring_off = [int(v) for v in np.asarray(ring_off).reshape(-1)]
    R = [tuple(int(v) for v in q) for q in np.asarray(ring_pts).reshape(-1, 2).tolist()]
    ring_group = [int(v) for v in np.asarray(ring_group).reshape(-1)]
    n, reach = len(off) - 1, int(reach)
    if not (1 <= reach <= REACH_MAX) or len(cls) != n or any(c < -1 for c in cls) or any(b < a for a, b in zip(ring_group, ring_group[1:])):
        raise ValueError("bad arguments")
    shapes = shape_edges(ring_off, R, ring_group)
    lines = [k for k in range(n) if off[k + 1] - off[k] == 2 and cls[k] >= 0]
    start = {k: P[off[k]] for k in lines}; end = {k: P[off[k] + 1] for k in lines}
    st = dict.fromkeys(STATS, 0)
    st["lines"] = len(lines)
    elig = []                                                        # (d2, a, b)
    for a in lines:
        e = end[a]
        e_inside = None
        for b in lines:
            if b <= a or cls[a] != cls[b]:
                continue
            s = start[b]
            dx, dy = s[0] - e[0], s[1] - e[1]
            if abs(dx) > reach or abs(dy) > reach or dx * dx + dy * dy > reach * reach:
                continue
            st["in_reach"] += 1
            edges = shapes.get(cls[a] >> 1, [])
            if e_inside is None:
                e_inside = inside(e, edges)
            if e_inside and not any(segments_meet(e, s, p, q) for p, q in edges):
                elig.append((dx * dx + dy * dy, a, b))
    st["eligible"] = len(elig)
    best_end, best_start = {}, {}
    for d2, a, b in elig:
        if a not in best_end or (d2, b) < best_end[a]:
            best_end[a] = (d2, b)
        if b not in best_start or (d2, a) < best_start[b]:
            best_start[b] = (d2, a)
    nxt = {a: b for a, (_, b) in best_end.items() if best_start[b][1] == a}
    has_prev = set(nxt.values())
    st["links"] = len(nxt)
    o_off, o_pts, m_off, member = [0], [], [0], []
    for k in range(n):
        if k in has_prev:
            continue
        if k not in start:                                            # takes no part
            o_pts += P[off[k]:off[k + 1]]; member.append(k)
        else:
            a = k
            o_pts += [start[a], end[a]]; member.append(a)
            while a in nxt:
                b = nxt[a]
                st["link_steps"] += max(abs(start[b][0] - end[a][0]), abs(start[b][1] - end[a][1]))
                if start[b] == o_pts[-1]:
                    st["coincident"] += 1
                else:
                    o_pts.append(start[b])
                o_pts.append(end[b]); member.append(b)
                a = b
        o_off.append(len(o_pts)); m_off.append(len(member))
    st["paths_out"], st["points_out"] = len(o_off) - 1, len(o_pts)
    return (np.asarray(o_off, np.int64), np.asarray(o_pts, np.int64).reshape(-1, 2).astype(np.int32), np.asarray(m_off, np.int64),
            np.asarray(member, np.int64).astype(np.int32), st)
