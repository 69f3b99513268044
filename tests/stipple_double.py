"""TEST INFRASTRUCTURE: the sequential double of --stipple-mm (include/orip.h: orip_gcode_stipple), in Python integers only.  For every shape it visits
every lattice point of the shape's bounding box, one after the other, and decides it by the rule's own words: INSIDE by orientation tests, CLEAR by the
three-case formula, then the rect, then the shapes above.  No scan line, no span, no chunk: nothing of the kernel's structure."""
import numpy as np

STATS = ("groups", "rows", "candidates", "near", "outside", "hidden", "dots")
SERPENTINE, OCCLUDE = 1, 2


def shapes_of(ring_off, ring_pts, ring_group):
    """group -> (the edges of positive length, all ring points), groups in input order (which ascends)"""
    out = {}
    for r, g in enumerate(ring_group):
        p = ring_pts[ring_off[r]:ring_off[r + 1]]
        edges, pts = out.setdefault(g, ([], []))
        pts.extend(p)
        edges.extend((a, b) for a, b in zip(p, p[1:] + p[:1]) if a != b)
    return out


def inside(P, edges):
    """even-odd; a point on an edge is not inside"""
    px, py = P
    par = 0
    for (ax, ay), (bx, by) in edges:
        cr = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        if cr == 0 and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by):
            return False
        if (ay <= py) != (by <= py) and (by > ay) == (cr > 0):            # the edge passes strictly to the right of P
            par ^= 1
    return bool(par)


def clear(P, edges, inset):
    px, py = P
    for (ax, ay), (bx, by) in edges:
        dx, dy, wx, wy = bx - ax, by - ay, px - ax, py - ay
        L, t = dx * dx + dy * dy, wx * dx + wy * dy
        if t <= 0:
            ok = wx * wx + wy * wy >= inset * inset
        elif t >= L:
            ok = (px - bx) ** 2 + (py - by) ** 2 >= inset * inset
        else:
            ok = (dx * wy - dy * wx) ** 2 >= inset * inset * L
        if not ok:
            return False
    return True


def stipple(ring_off, ring_pts, ring_group, lattice, inset, rect, flags):
    """-> (xy int32 [dots, 2], group int32 [dots], {STATS})"""
    ring_off = np.asarray(ring_off, np.int64).reshape(-1).tolist()
    ring_pts = [tuple(q) for q in np.asarray(ring_pts, np.int64).reshape(-1, 2).tolist()]
    ring_group = np.asarray(ring_group, np.int64).reshape(-1).tolist()
    p, q, s = (int(v) for v in lattice)
    x0, y0, x1, y1 = (int(v) for v in rect)
    inset = int(inset)
    shapes = shapes_of(ring_off, ring_pts, ring_group)
    st = dict.fromkeys(STATS, 0)
    xy, grp = [], []
    for g in sorted(shapes):
        edges, pts = shapes[g]
        if not edges:
            continue
        st["groups"] += 1
        bx0, by0, bx1, by1 = min(v[0] for v in pts), min(v[1] for v in pts), max(v[0] for v in pts), max(v[1] for v in pts)
        for j in range(-((-by0) // q), by1 // q + 1):
            st["rows"] += 1
            sh = s if j & 1 else 0
            xs = [i * p + sh for i in range(-((-(bx0 - sh)) // p), (bx1 - sh) // p + 1)]
            if flags & SERPENTINE and j & 1:
                xs.reverse()
            for x in xs:
                P = (x, j * q)
                if not inside(P, edges):
                    continue
                st["candidates"] += 1
                if not clear(P, edges, inset):
                    st["near"] += 1
                elif not (x0 <= P[0] <= x1 and y0 <= P[1] <= y1):
                    st["outside"] += 1
                elif flags & OCCLUDE and any(h > g and inside(P, shapes[h][0]) for h in shapes):
                    st["hidden"] += 1
                else:
                    st["dots"] += 1; xy.append(P); grp.append(g)
    return np.asarray(xy, np.int32).reshape(-1, 2), np.asarray(grp, np.int32).reshape(-1), st
