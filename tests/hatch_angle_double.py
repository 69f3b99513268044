"""TEST INFRASTRUCTURE: the hatch at an angle (include/orip.h: orip_svg_hatch_angle) as the rule states it, sequential, in Python integers and Fractions:
one loop over the families, the groups, the edges and the lines, nothing vectorised and nothing shared with csrc/hatch_angle.hip, so that the kernels can
be held to it by equality.  Slow on purpose: the drawings of the tests keep a group to a few dozen lines."""
from fractions import Fraction
from math import isqrt

import numpy as np

from svg_double import round4_python

SERPENTINE, HORIZONTAL, VERTICAL = 1, 2, 4
QLIM = 1 << 24
UMAX = 4096
MAX_ROWS, MAX_CROSSINGS = 1 << 26, 1 << 30


def rs(v):
    """the nearest integer to sqrt(v), exactly"""
    return (isqrt(4 * v) + 1) >> 1


def half_up(f):
    """the nearest integer to the Fraction f, halves toward +infinity"""
    return (2 * f.numerator + f.denominator) // (2 * f.denominator)


def hatch_family(off, q, gid, spacing, inset, u, serpentine):
    """one family of lines along u -> (rows (x0, y0, x1, y1), the group of every row, the line k of every row, lines, crossings, collapsed)"""
    ux, uy = int(u[0]), int(u[1])
    U2 = ux * ux + uy * uy
    D, I = rs(spacing * spacing * U2), rs(inset * inset * U2)
    seg, grp, ks, lines, crossings, collapsed = [], [], [], 0, 0, 0
    for g in sorted(set(int(v) for v in gid if v >= 0)):
        subs = [[(int(x), int(y)) for x, y in q[off[p]:off[p + 1]]] for p in range(len(gid)) if gid[p] == g]
        s_all = [-uy * x + ux * y for sub in subs for x, y in sub]
        if not s_all:
            continue
        klo, khi = min(s_all) // D + 1, max(s_all) // D
        lines += max(0, khi - klo + 1)
        if lines > MAX_ROWS:
            raise ValueError("more than 2^26 hatch lines")
        rows = {}
        for sub in subs:
            for i in range(len(sub)):
                a, b = sub[i], sub[(i + 1) % len(sub)]
                sa, sb = -uy * a[0] + ux * a[1], -uy * b[0] + ux * b[1]
                wa, wb = ux * a[0] + uy * a[1], ux * b[0] + uy * b[1]
                if sa == sb:
                    continue
                if sa > sb:
                    sa, sb, wa, wb = sb, sa, wb, wa
                for k in range(sa // D + 1, sb // D + 1):                    # sa < k D <= sb
                    rows.setdefault(k, []).append(Fraction(wa * (sb - sa) + (k * D - sa) * (wb - wa), sb - sa))
                    crossings += 1
        for k in range(klo, khi + 1):
            ws_ = sorted(rows.get(k, []))
            for j in range(0, len(ws_) - 1, 2):
                ws, we = ws_[j] + I, ws_[j + 1] - I
                if not we > ws:
                    continue
                p0 = (half_up((ws * ux - k * D * uy) / U2), half_up((ws * uy + k * D * ux) / U2))
                p1 = (half_up((we * ux - k * D * uy) / U2), half_up((we * uy + k * D * ux) / U2))
                if p0 == p1:
                    collapsed += 1
                    continue
                if serpentine and (k & 1):
                    p0, p1 = p1, p0
                seg.append(p0 + p1); grp.append(g); ks.append(k)
    if crossings > MAX_CROSSINGS:
        raise ValueError("more than 2^30 crossings")
    return seg, grp, ks, lines, crossings, collapsed


def hatch_lines_angle(off, q, fill_group, spacing, inset, u, flags):
    """-> (segments int64 [S, 4], counts, the group of every segment, the line k of every segment, the family's u of every segment)"""
    ux, uy = int(u[0]), int(u[1])
    if spacing < 1 or inset < 0 or not flags & (HORIZONTAL | VERTICAL) or flags & ~7:
        raise ValueError("bad hatch parameters")
    if (ux == 0 and uy == 0) or max(abs(ux), abs(uy)) > UMAX:
        raise ValueError("hatch direction out of range")
    off = [int(v) for v in np.asarray(off, np.int64)]
    q = np.asarray(q, np.int64).reshape(-1, 2)
    if len(q) and int(np.abs(q).max()) >= QLIM:
        raise ValueError("a coordinate reaches 2^24 steps")
    gid = [int(v) for v in np.asarray(fill_group, np.int64).reshape(-1)]
    if len(gid) != len(off) - 1 or any(v < -1 or v >= len(gid) for v in gid):
        raise ValueError("fill group out of range")
    seg, grp, ks, us, st = [], [], [], [], {"groups": len(set(v for v in gid if v >= 0)), "lines": 0, "crossings": 0, "segments": 0, "collapsed": 0}
    for bit, fu in ((HORIZONTAL, (ux, uy)), (VERTICAL, (-uy, ux))):
        if flags & bit:
            s, g, k, lines, cross, coll = hatch_family(off, q, gid, int(spacing), int(inset), fu, bool(flags & SERPENTINE))
            seg += s; grp += g; ks += k; us += [fu] * len(s)
            st["lines"] += lines; st["crossings"] += cross; st["collapsed"] += coll
    st["segments"] = len(seg)
    return np.asarray(seg, np.int64).reshape(-1, 4), st, np.asarray(grp, np.int32), np.asarray(ks, np.int64), np.asarray(us, np.int64).reshape(-1, 2)


def hatch_segments_angle(off, q, fill_group, spacing, inset, u, flags):
    """every family the flags ask for, the one along u first -> (segments int64 [S, 4], {"groups", "lines", "crossings", "segments", "collapsed"})"""
    return hatch_lines_angle(off, q, fill_group, spacing, inset, u, flags)[:2]


def quantise(pts_mm, steps_per_mm):
    with np.errstate(all="ignore"):
        q = np.rint(np.asarray(pts_mm, np.float64).reshape(-1, 2) * float(steps_per_mm))
    if not (np.abs(q) < QLIM).all():
        raise ValueError("a coordinate reaches 2^24 steps")
    return q.astype(np.int64)


class HatchAngleWithGroups:
    """stand-in for orip.svg._Resident.hatch (routed on "u") and .hatch_groups on (off, pts) paths in page mm: the hatch lines behind them as 2-point paths,
    and the fill group of every one"""
    def __init__(self): self.groups = np.zeros(0, np.int32)

    def hatch(self, paths, fill_group, prm):
        off, pts = np.asarray(paths[0], np.int64), np.asarray(paths[1], np.float64).reshape(-1, 2)
        spm = float(prm["steps_per_mm"])
        if not 0.0 < spm <= 5000.0:
            raise ValueError("steps per mm out of range for hatching")
        seg, st, grp, _, _ = hatch_lines_angle(off, quantise(pts, spm), fill_group, prm["spacing"], prm["inset"], prm["u"], prm["flags"])
        self.groups = grp
        mm = round4_python(seg.reshape(-1, 2).astype(np.float64) / spm)
        return (np.concatenate([off, off[-1] + 2 * np.arange(1, len(seg) + 1)]), np.concatenate([pts, mm.reshape(-1, 2)])), st

    def hatch_groups(self, paths, segments):
        assert segments == len(self.groups)
        return self.groups


def hatch_angle_numpy(paths, fill_group, prm):
    """stand-in for orip.svg._Resident.hatch alone"""
    return HatchAngleWithGroups().hatch(paths, fill_group, prm)
