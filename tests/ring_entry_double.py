"""TEST INFRASTRUCTURE: --ring-entry by the rule of include/orip.h (orip_gcode_order_rings), with no knowledge of the kernel: a sequential walk that takes, at
every step, the minimum of (L1 distance, stroke, candidate) over every candidate of every remaining stroke of the group.  Distances are int64 (at most
2^31); the candidates lie in one flat table sorted by (stroke, candidate), so the first of the minima numpy's argmin returns is the rule's tie-break."""
import numpy as np

STAT_NAMES = ("closed", "moved", "candidates", "travel")


def is_closed(P):
    return len(P) >= 4 and int(P[0][0]) == int(P[-1][0]) and int(P[0][1]) == int(P[-1][1])


def candidates(off, pts, reverse):
    """(stroke, c, x, y) of every candidate, in (stroke, c) order, and which strokes are closed"""
    off = np.asarray(off, np.int64).reshape(-1); pts = np.asarray(pts, np.int64).reshape(-1, 2)
    rows, closed = [], []
    for i in range(len(off) - 1):
        P = pts[off[i]:off[i + 1]]
        closed.append(is_closed(P))
        if closed[-1]:
            rows += [(i, v, int(P[v][0]), int(P[v][1])) for v in range(len(P) - 1)]
        else:
            rows.append((i, 0, int(P[0][0]), int(P[0][1])))
            if reverse:
                rows.append((i, 1, int(P[-1][0]), int(P[-1][1])))
    return np.asarray(rows, np.int64).reshape(-1, 4), np.asarray(closed, bool)


def order_rings(off, pts, group=None, n_groups=1, reverse=False, start=(0, 0)):
    """-> (order int32 [n], rev bool [n], seam int32 [n] by sequence position, stats)"""
    off = np.asarray(off, np.int64).reshape(-1); pts = np.asarray(pts, np.int64).reshape(-1, 2)
    n = len(off) - 1
    grp = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64).reshape(-1)
    C, closed = candidates(off, pts, reverse)
    order, rev, seam = np.zeros(n, np.int32), np.zeros(n, bool), np.zeros(n, np.int32)
    cx, cy = int(start[0]), int(start[1])
    travel, k = 0, 0
    far = np.iinfo(np.int64).max
    for g in range(int(n_groups)):
        T = C[grp[C[:, 0]] == g] if len(C) else C
        alive = np.ones(len(T), bool)
        for _ in range(int((grp == g).sum())):
            d = np.where(alive, np.abs(T[:, 2] - cx) + np.abs(T[:, 3] - cy), far)
            j = int(np.argmin(d))                        # the first of the minima: the lowest (stroke, candidate)
            i, c, x, y = (int(v) for v in T[j])
            travel += max(abs(x - cx), abs(y - cy))
            order[k] = i
            if closed[i]:
                seam[k] = c; cx, cy = x, y
            else:
                rev[k] = bool(c)
                cx, cy = (int(v) for v in (pts[off[i]] if c else pts[off[i + 1] - 1]))
            alive &= T[:, 0] != i
            k += 1
    return order, rev, seam, dict(closed=int(closed.sum()), moved=int((seam != 0).sum()), candidates=len(C), travel=travel)


def order_rings_fn(off, pts, group, n_groups, reverse):
    """the double in the form of GcodeOptions' ring_entry_fn"""
    return order_rings(off, pts, group, n_groups, reverse)
