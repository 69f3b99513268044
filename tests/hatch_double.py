"""TEST INFRASTRUCTURE: a numpy restatement of the hatch fill (include/orip.h: orip_svg_hatch), written from the rules and vectorised over all edges and
lines at once, so that the kernels of csrc/hatch.hip can be checked against something that shares no code with them, and the host logic of orip/svg.py on
the CPU.  It is itself held to the reference's hatch_fill by the recorded calls of tests/golden/golden_hatch.npz (test_hatch_host.py)."""
import numpy as np

from svg_double import round4_python

SERPENTINE, HORIZONTAL, VERTICAL = 1, 2, 4
QLIM = 1 << 30
MAX_ROWS, MAX_CROSSINGS = 1 << 26, 1 << 30


def hatch_direction(off, q, gid, spacing, inset, serpentine, vert=False):
    """off int64 [P + 1], q integer points [N, 2], gid [P] (-1 or a group number; the groups go in ascending order) ->
    (segments int64 [S, 4] as (x0, y0, x1, y1) in output order, lines, crossings)"""
    off = np.asarray(off, np.int64); q = np.asarray(q, np.int64).reshape(-1, 2); gid = np.asarray(gid, np.int64)
    spacing, inset = int(spacing), int(inset)
    if vert:
        q = q[:, ::-1]
    none = np.zeros((0, 4), np.int64)
    lens = np.diff(off)
    used = np.unique(gid[gid >= 0])
    if len(used) == 0 or len(q) == 0:
        return none, 0, 0
    rank = np.full(len(gid), -1, np.int64); rank[gid >= 0] = np.searchsorted(used, gid[gid >= 0])
    pg = np.repeat(rank, lens)                                   # group of every point
    G = len(used)
    j = np.arange(len(q))
    nxt = j + 1
    nxt[off[1:][lens > 0] - 1] = off[:-1][lens > 0]               # the last point of a subpath goes back to its first
    inside = pg >= 0
    ymin = np.full(G, np.iinfo(np.int64).max); ymax = np.full(G, np.iinfo(np.int64).min)
    np.minimum.at(ymin, pg[inside], q[inside, 1]); np.maximum.at(ymax, pg[inside], q[inside, 1])
    y0 = (ymin + spacing // 2) // spacing * spacing
    nl = np.where(ymax >= y0, (ymax - y0) // spacing + 1, 0)
    rowbase = np.concatenate([[0], np.cumsum(nl)])
    if rowbase[-1] > MAX_ROWS:
        raise ValueError("more than 2^26 hatch lines")
    a, b = q[j], q[nxt]
    e = np.nonzero(inside & (a[:, 1] != b[:, 1]))[0]
    a, b, g = a[e], b[e], pg[e]
    sw = a[:, 1] > b[:, 1]
    a, b = np.where(sw[:, None], b, a), np.where(sw[:, None], a, b)
    klo = np.maximum(0, (a[:, 1] - y0[g]) // spacing + 1)
    khi = (b[:, 1] - y0[g]) // spacing
    cnt = np.maximum(0, khi - klo + 1)
    X = int(cnt.sum())
    if X > MAX_CROSSINGS:
        raise ValueError("more than 2^30 crossings")
    if X == 0:
        return none, int(rowbase[-1]), 0
    ei = np.repeat(np.arange(len(e)), cnt)
    k = klo[ei] + (np.arange(X) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    y = y0[g[ei]] + k * spacing
    x1, y1, x2, y2 = a[ei, 0], a[ei, 1], b[ei, 0], b[ei, 1]
    t = (y - y1).astype(np.float64) / (y2 - y1).astype(np.float64)
    x = x1.astype(np.float64) + t * (x2 - x1).astype(np.float64)
    row = rowbase[g[ei]] + k
    o = np.lexsort((x, row))
    x, row, k, y = x[o], row[o], k[o], y[o]
    start = np.searchsorted(row, row, "left")
    li = np.arange(X) - start
    first = np.nonzero((li % 2 == 0) & (np.arange(X) + 1 < X) & (np.append(row[1:], -1) == row))[0]
    sx = np.trunc(x[first] + float(inset)).astype(np.int64); ex = np.trunc(x[first + 1] - float(inset)).astype(np.int64)
    kept = ex > sx
    sx, ex, yk, kk = sx[kept], ex[kept], y[first][kept], k[first][kept]
    rev = (kk % 2 == 1) if serpentine else np.zeros(len(kk), bool)
    p0, p1 = np.where(rev, ex, sx), np.where(rev, sx, ex)
    seg = np.stack([yk, p0, yk, p1], 1) if vert else np.stack([p0, yk, p1, yk], 1)
    return seg, int(rowbase[-1]), X


def hatch_segments(off, q, gid, spacing, inset, flags):
    """every direction the flags ask for, horizontal first -> (segments int64 [S, 4], {"groups", "lines", "crossings", "segments"})"""
    if spacing < 1 or inset < 0 or not flags & (HORIZONTAL | VERTICAL):
        raise ValueError("bad hatch parameters")
    gid = np.asarray(gid, np.int64)
    if ((gid < -1) | (gid >= len(gid))).any():
        raise ValueError("fill group out of range")
    out, lines, cross = [], 0, 0
    for bit, vert in ((HORIZONTAL, False), (VERTICAL, True)):
        if flags & bit:
            s, l, x = hatch_direction(off, q, gid, spacing, inset, bool(flags & SERPENTINE), vert)
            out.append(s); lines += l; cross += x
    seg = np.concatenate(out) if out else np.zeros((0, 4), np.int64)
    return seg, {"groups": int(len(np.unique(gid[gid >= 0]))), "lines": lines, "crossings": cross, "segments": len(seg)}


def quantise(pts_mm, steps_per_mm):
    with np.errstate(all="ignore"):
        q = np.rint(np.asarray(pts_mm, np.float64).reshape(-1, 2) * float(steps_per_mm))
    if not (np.abs(q) < QLIM).all():
        raise ValueError("a coordinate reaches 2^30 hatch units")
    return q.astype(np.int64)


def hatch_numpy(paths, fill_group, prm):
    """stand-in for orip.svg._Resident.hatch on (off, pts) paths in page mm: the hatch lines behind them as 2-point paths -> ((off, pts), counts)"""
    off, pts = np.asarray(paths[0], np.int64), np.asarray(paths[1], np.float64).reshape(-1, 2)
    spm = float(prm["steps_per_mm"])
    if not 0.0 < spm <= 5000.0:
        raise ValueError("steps per mm out of range for hatching")
    if len(fill_group) != len(off) - 1:
        raise ValueError("one fill group per path")
    seg, st = hatch_segments(off, quantise(pts, spm), fill_group, prm["spacing"], prm["inset"], prm["flags"])
    mm = round4_python(seg.reshape(-1, 2).astype(np.float64) / spm)
    return (np.concatenate([off, off[-1] + 2 * np.arange(1, len(seg) + 1)]), np.concatenate([pts, mm.reshape(-1, 2)])), st


def polys_table(polys_by_group, fill=True):
    """integer polygons (a list of groups, each a list of [n, 2] arrays) as a SegmentTable of line subpaths under the identity: the way polyline_table of
    test_gpu_svg.py puts arbitrary values on the device; one subpath per polygon, fill_group = its group"""
    from orip.svg import SegmentTable
    ctrl, sub, fg = [], [0], []
    for g, polys in enumerate(polys_by_group):
        for poly in polys:
            p = np.asarray(poly, np.float64).reshape(-1, 2)
            ctrl.append(np.stack([p[:-1], p[1:], p[1:], p[1:]], 1)); sub.append(sub[-1] + len(p) - 1); fg.append(g if fill else -1)
    ctrl = np.concatenate(ctrl)
    return SegmentTable(np.ones(len(ctrl), np.int32), ctrl, np.zeros(len(ctrl), np.int32), np.array(sub, np.int64), np.zeros(len(fg), np.uint8),
                        np.array([[1.0, 0.0, 0.0, -1.0, 0.0, 0.0]]), 0.0, np.array(fg, np.int32))


def star(rng, cx, cy, r, n):
    """a star polygon of n integer vertices around (cx, cy), radii between 0.3 r and r"""
    ang = np.sort(rng.uniform(0, 2 * np.pi, n)); rad = rng.uniform(0.3, 1.0, n) * r
    return np.stack([np.rint(cx + rad * np.cos(ang)), np.rint(cy + rad * np.sin(ang))], 1).astype(np.int64)


def single_polygon(n_edges=100000, w=8400, h=11880, seed=5):
    """one polygon of n_edges integer vertices filling an A4 page in steps: a wobbling outline, so that every hatch line crosses it many times"""
    rng = np.random.default_rng(seed)
    ang = np.arange(n_edges) * (2 * np.pi / n_edges)
    rad = 0.35 + 0.1 * np.sin(40 * ang) + rng.uniform(-0.02, 0.02, n_edges)
    return np.stack([np.rint(w / 2 + rad * w * np.cos(ang)), np.rint(h / 2 + rad * h * np.sin(ang))], 1).astype(np.int64)
