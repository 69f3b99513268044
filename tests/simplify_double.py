"""TEST INFRASTRUCTURE: the sequential double of orip_gcode_simplify (include/orip.h states the rule): Ramer-Douglas-Peucker per stroke with an explicit
stack, every coordinate a Python integer (arbitrary precision), no numpy arithmetic on coordinates.  Not the product: the product has no CPU path."""
import numpy as np

TOL4_MAX = (1 << 17) - 1
TOP = 1 << 30


def key(A, B, P):
    """(K, L) of the interior point P in the span with ends A, B: the squared distance to the segment times L; L == 0: the squared distance to the point"""
    dx, dy = B[0] - A[0], B[1] - A[1]
    px, py = P[0] - A[0], P[1] - A[1]
    L = dx * dx + dy * dy
    if L == 0:
        return px * px + py * py, 0
    t = px * dx + py * dy
    if t <= 0:
        return (px * px + py * py) * L, L
    if t >= L:
        qx, qy = P[0] - B[0], P[1] - B[1]
        return (qx * qx + qy * qy) * L, L
    cr = px * dy - py * dx
    return cr * cr, L


def within(A, B, P, tol4):
    """P is within the tolerance of the segment A B (a degenerate one: on the point)"""
    K, L = key(A, B, P)
    return K == 0 if L == 0 else 16 * K <= tol4 * tol4 * L


def simplify_stroke(P, tol4):
    """indices of the kept points of one stroke, P a list of (x, y) Python integers"""
    keep = [False] * len(P)
    keep[0] = keep[-1] = True
    stack = [(0, len(P) - 1)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        bestK, m, L = -1, -1, 0
        for i in range(a + 1, b):
            K, L = key(P[a], P[b], P[i])
            if K > bestK:
                bestK, m = K, i
        if (bestK > 0) if L == 0 else (16 * bestK > tol4 * tol4 * L):
            keep[m] = True
            stack.append((a, m)); stack.append((m, b))
    return [i for i, k in enumerate(keep) if k]


def check_input(off, pts, tol4):
    off = np.asarray(off, np.int64).reshape(-1); pts = np.asarray(pts, np.int64).reshape(-1, 2)
    if not (0 <= int(tol4) <= TOL4_MAX):
        raise ValueError("tol4 0..2^17 - 1")
    if len(off) < 1 or off[0] != 0 or (np.diff(off) < 2).any() or int(off[-1]) != len(pts):
        raise ValueError("offsets")
    if len(pts) and (pts.min() < 0 or pts.max() > TOP):
        raise ValueError("coordinate outside 0..2^30")
    same = (pts[1:] == pts[:-1]).all(1)
    same[off[1:-1] - 1] = False                                               # the last point of a stroke and the first of the next may be equal
    if same.any():
        raise ValueError("a point equals the point before it")
    return off, pts


def simplify_numpy(off, pts, tol4):
    """what orip.device.Device.gcode_simplify returns: (off int64, pts int32 [total', 2], kept int64 [total'], stats); rounds is the device's own business (0)"""
    off, pts = check_input(off, pts, tol4)
    tol4 = int(tol4)
    flat = pts.tolist()
    kept, noff = [], [0]
    for p in range(len(off) - 1):
        a, b = int(off[p]), int(off[p + 1])
        kept += [a + i for i in simplify_stroke([tuple(q) for q in flat[a:b]], tol4)]
        noff.append(len(kept))
    kept = np.asarray(kept, np.int64).reshape(-1)
    out = np.ascontiguousarray(np.asarray(pts, np.int32).reshape(-1, 2)[kept]).reshape(-1, 2)
    return np.asarray(noff, np.int64), out, kept, {"paths": len(off) - 1, "points_in": len(pts), "points_out": len(kept), "rounds": 0}
