"""TEST INFRASTRUCTURE: --loop-start by the rule of include/orip.h (orip_gcode_seam), with no knowledge of the kernel: the cost-to-go of every ring vertex
taken backwards over the whole sequence, then the lowest vertex that attains the minimum taken forwards.  Integers throughout: Python's own where a stroke
is small, numpy int64 for the minimum over a ring (exact: a value is a sum of at most n distances of at most 2^30, n <= 2^26).  exhaustive() tries every
assignment of seams of a tiny input and is what the double itself is checked against; travel() walks the polylines as they would be drawn."""
import itertools

import numpy as np

STAT_NAMES = ("closed", "moved", "travel_before", "travel_after")


def dist(p, q):
    return max(abs(int(p[0]) - int(q[0])), abs(int(p[1]) - int(q[1])))


def strokes_of(off, pts, order=None):
    """the point lists of the strokes in drawing order"""
    off = np.asarray(off, np.int64).reshape(-1); pts = np.asarray(pts, np.int64).reshape(-1, 2)
    seq = range(len(off) - 1) if order is None else [int(p) for p in order]
    return [pts[off[p]:off[p + 1]] for p in seq]


def is_closed(P):
    return len(P) >= 4 and int(P[0][0]) == int(P[-1][0]) and int(P[0][1]) == int(P[-1][1])


def drawn(P, s, r):
    """the stroke as drawn with seam s and direction r: rotated in the stored list, then turned round"""
    P = np.asarray(P, np.int64)
    if s:
        L = len(P)
        P = P[(s + np.arange(L)) % (L - 1)]
    return P[::-1] if r else P


def travel(off, pts, order=None, rev=None, seam=None, start=(0, 0)):
    """pen-up steps of the sequence from `start`, recomputed from the polylines as drawn"""
    S = strokes_of(off, pts, order)
    cur, total = (int(start[0]), int(start[1])), 0
    for k, P in enumerate(S):
        Q = drawn(P, 0 if seam is None else int(seam[k]), bool(rev[k]) if rev is not None else False)
        total += dist(cur, Q[0])
        cur = (int(Q[-1][0]), int(Q[-1][1]))
    return total


def _layer(V, U, g):
    """min_u d(v, u) + g[u] for every v, in blocks of rows"""
    out = np.empty(len(V), np.int64)
    for a in range(0, len(V), 256):
        d = np.abs(V[a:a + 256, None, :] - U[None, :, :]).max(2)
        out[a:a + 256] = (d + g[None, :]).min(1)
    return out


def seams(off, pts, order=None, rev=None, start=(0, 0)):
    """(seam int32 [n] by sequence position, stats)"""
    S = strokes_of(off, pts, order)
    n = len(S)
    rv = [False] * n if rev is None else [bool(r) for r in rev]
    closed = [is_closed(P) for P in S]
    entry = [None if closed[k] else (S[k][-1] if rv[k] else S[k][0]) for k in range(n)]
    leave = [None if closed[k] else (S[k][0] if rv[k] else S[k][-1]) for k in range(n)]
    f = [None] * n                                       # f[k][v]: the travel behind stroke k when it is left at ring vertex v
    for k in range(n - 1, -1, -1):
        if not closed[k]:
            continue
        V = S[k][:-1]
        if k == n - 1:
            f[k] = np.zeros(len(V), np.int64)
        elif closed[k + 1]:
            f[k] = _layer(V, S[k + 1][:-1], f[k + 1])
        else:
            f[k] = np.abs(V - entry[k + 1][None, :]).max(1)      # what follows an open stroke is the same for every v: left out
    seam = np.zeros(n, np.int32)
    cur = np.asarray(start, np.int64)
    for k in range(n):
        if closed[k]:
            cost = np.abs(S[k][:-1] - cur[None, :]).max(1) + f[k]
            seam[k] = int(np.argmin(cost))               # the first of the minima: the lowest vertex
            cur = S[k][seam[k]]
        else:
            cur = leave[k]
    st = dict(closed=int(sum(closed)), moved=int((seam != 0).sum()), travel_before=travel(off, pts, order, rev, None, start),
              travel_after=travel(off, pts, order, rev, seam, start))
    return seam, st


def exhaustive(off, pts, order=None, rev=None, start=(0, 0)):
    """(least travel, the lexicographically smallest seam list that has it), every assignment tried: for tiny inputs"""
    S = strokes_of(off, pts, order)
    choices = [range(len(P) - 1) if is_closed(P) else (0,) for P in S]
    best = None
    for cand in itertools.product(*choices):             # in lexicographic order: the first of the best is the smallest
        t = travel(off, pts, order, rev, cand, start)
        if best is None or t < best[0]:
            best = (t, list(cand))
    return best
