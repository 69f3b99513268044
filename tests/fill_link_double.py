"""Sequential double of orip_fill_link (include/orip.h states the rule): plain Python integers over ALL pairs of segments -- no window, no row index, no
binary search.  The line (family, k) of every segment comes from this file's own runs of tests/fill_double.py, one per family.  fill_link_numpy, at the
end, is the same rule over arrays for the input that exceeds a launch cap, and is held to fill_link by equality on the small cases."""
import numpy as np

import fill_double as FD

STATS = ("segments", "in_reach", "eligible", "links", "paths_out", "points_out", "link_steps")


def lines_of(seg, u, spacing):
    """k of every segment of the family u: the nearest line to its START (|n.P - k D| <= m / 2 < D / 2, so there is one)"""
    D = FD.frame(u, spacing, 0, 1)[1]
    return [(2 * (-u[1] * int(x) + u[0] * int(y)) + D) // (2 * D) for x, y in np.asarray(seg)[:, :2].tolist()]


def segments_with_lines(mask, W, H, place, u, spacing, inset, min_len, flags, fill=FD.fill_mask):
    """-> (seg int32 [n, 4] as orip_fill_mask leaves them, [(family, k)] per segment): the families one by one, which is the order of the whole"""
    u = (int(u[0]), int(u[1]))
    segs, fk = [], []
    for f, (bit, uf) in enumerate(((FD.ALONG, u), (FD.ACROSS, (-u[1], u[0])))):
        if flags & bit:
            s = fill(mask, W, H, place, u, spacing, inset, min_len, (flags & FD.SERPENTINE) | bit)[0]
            segs.append(s)
            fk += [(f, k) for k in lines_of(s, uf, spacing)]
    return np.concatenate(segs).astype(np.int32).reshape(-1, 4), fk


def link_pixels(E, S):
    """the pixels t = 0 .. n of the link E -> S"""
    dx, dy = S[0] - E[0], S[1] - E[1]
    n = max(abs(dx), abs(dy))
    assert n >= 1
    out = []
    for t in range(n + 1):
        if abs(dx) >= abs(dy):
            out.append((E[0] + (t if dx > 0 else -t), E[1] + (2 * t * dy + n) // (2 * n)))
        else:
            out.append((E[0] + (2 * t * dx + n) // (2 * n), E[1] + (t if dy > 0 else -t)))
    return out


def chains(S, nxt, prv, seg):
    """-> (off int64 [paths + 1], pts int32 [2 S, 2], members per stroke)"""
    off, pts, members = [0], [], []
    for j in range(S):
        if prv[j] is not None:
            continue
        m = []
        while j is not None:
            m.append(j)
            pts += [seg[j][0:2], seg[j][2:4]]
            j = nxt[j]
        members.append(m)
        off.append(len(pts))
    return np.asarray(off, np.int64), np.asarray(pts, np.int32).reshape(-1, 2), members


def fill_link(mask, W, H, place, u, spacing, inset, min_len, flags, reach, detail=None):
    """-> (off int64 [paths_out + 1], pts int32 [points_out, 2], {STATS}); detail, a dict, receives seg, fk, the links and the members of every stroke"""
    assert 1 <= reach <= 1 << 15
    M = np.asarray(mask)
    place = tuple(int(v) for v in place)
    seg, fk = segments_with_lines(M, W, H, place, u, spacing, inset, min_len, flags)
    seg = seg.tolist()
    S = len(seg)
    st = dict.fromkeys(STATS, 0)
    st["segments"] = S
    best_out, best_in = [None] * S, [None] * S
    for a in range(S):
        for b in range(S):
            if fk[a][0] != fk[b][0] or fk[b][1] != fk[a][1] + 1:
                continue
            E, B = (seg[a][2], seg[a][3]), (seg[b][0], seg[b][1])
            dx, dy = B[0] - E[0], B[1] - E[1]
            if max(abs(dx), abs(dy)) > reach or dx * dx + dy * dy > reach * reach:
                continue
            st["in_reach"] += 1
            if not all(FD.ink(M, place, X, Y) for X, Y in link_pixels(E, B)):
                continue
            st["eligible"] += 1
            d2 = dx * dx + dy * dy
            if best_out[a] is None or (d2, b) < best_out[a]:
                best_out[a] = (d2, b)
            if best_in[b] is None or (d2, a) < best_in[b]:
                best_in[b] = (d2, a)
    nxt, prv = [None] * S, [None] * S
    for a in range(S):
        if best_out[a] is not None and best_in[best_out[a][1]][1] == a:
            b = best_out[a][1]
            assert a < b
            nxt[a], prv[b] = b, a
            st["links"] += 1
            st["link_steps"] += max(abs(seg[b][0] - seg[a][2]), abs(seg[b][1] - seg[a][3]))
    off, pts, members = chains(S, nxt, prv, seg)
    st["paths_out"], st["points_out"] = len(off) - 1, len(pts)
    if detail is not None:
        detail.update(seg=np.asarray(seg, np.int32).reshape(-1, 4), fk=fk, links=[(a, nxt[a]) for a in range(S) if nxt[a] is not None], members=members)
    return off, pts, st


def fill_link_numpy(mask, W, H, place, u, spacing, inset, min_len, flags, reach):
    """fill_link once more over arrays, for inputs of tens of thousands of segments: the pairs are formed line against next line (every other pair fails
    the first condition of "in reach"), the link pixels as one padded array.  Pinned to fill_link by equality (tests/test_fill_link_host.py)."""
    M = np.asarray(mask) != 0
    num, den, ox, oy = (int(v) for v in place)
    seg, fk = segments_with_lines(mask, W, H, place, u, spacing, inset, min_len, flags, fill=FD.fill_mask_numpy)
    seg = seg.astype(np.int64)
    S = len(seg)
    st = dict.fromkeys(STATS, 0)
    st["segments"] = S
    fk = np.asarray(fk, np.int64).reshape(-1, 2)
    A, B = [], []
    for key in sorted(set(map(tuple, fk.tolist()))):
        ia = np.nonzero((fk[:, 0] == key[0]) & (fk[:, 1] == key[1]))[0]
        ib = np.nonzero((fk[:, 0] == key[0]) & (fk[:, 1] == key[1] + 1))[0]
        if len(ia) and len(ib):
            dx = seg[ib, 0][None, :] - seg[ia, 2][:, None]
            dy = seg[ib, 1][None, :] - seg[ia, 3][:, None]
            pa, pb = np.nonzero((np.maximum(np.abs(dx), np.abs(dy)) <= reach) & (dx * dx + dy * dy <= reach * reach))
            A.append(ia[pa]); B.append(ib[pb])
    A = np.concatenate(A) if A else np.zeros(0, np.int64)
    B = np.concatenate(B) if B else np.zeros(0, np.int64)
    st["in_reach"] = len(A)
    nxt, prv = np.full(S, -1, np.int64), np.full(S, -1, np.int64)
    if len(A):
        Ex, Ey = seg[A, 2], seg[A, 3]
        dx, dy = seg[B, 0] - Ex, seg[B, 1] - Ey
        n = np.maximum(np.abs(dx), np.abs(dy))
        assert (n >= 1).all()
        t = np.arange(int(n.max()) + 1, dtype=np.int64)[None, :]
        live = t <= n[:, None]
        tt = np.minimum(t, n[:, None])
        xm = (np.abs(dx) >= np.abs(dy))[:, None]
        n2 = n[:, None]
        X = Ex[:, None] + np.where(xm, np.sign(dx)[:, None] * tt, (2 * tt * dx[:, None] + n2) // (2 * n2))
        Y = Ey[:, None] + np.where(xm, (2 * tt * dy[:, None] + n2) // (2 * n2), np.sign(dy)[:, None] * tt)
        c, r = ((X - ox) * den) // num, ((Y - oy) * den) // num
        ok = (c >= 0) & (c < M.shape[1]) & (r >= 0) & (r < M.shape[0])
        ink = np.zeros(X.shape, bool)
        ink[ok] = M[r[ok], c[ok]]
        el = (ink | ~live).all(1)
        A, B, d2 = A[el], B[el], (dx * dx + dy * dy)[el]
        st["eligible"] = len(A)
        best_out, best_in = np.full(S, -1, np.int64), np.full(S, -1, np.int64)
        o = np.lexsort((B, d2, A))                                                    # per a: the least (d2, b) comes first
        first = np.r_[True, A[o][1:] != A[o][:-1]] if len(o) else np.zeros(0, bool)
        best_out[A[o][first]] = B[o][first]
        o = np.lexsort((A, d2, B))
        first = np.r_[True, B[o][1:] != B[o][:-1]] if len(o) else np.zeros(0, bool)
        best_in[B[o][first]] = A[o][first]
        a = np.nonzero(best_out >= 0)[0]
        a = a[best_in[best_out[a]] == a]
        nxt[a] = best_out[a]; prv[best_out[a]] = a
        st["links"] = len(a)
        st["link_steps"] = int(np.maximum(np.abs(seg[nxt[a], 0] - seg[a, 2]), np.abs(seg[nxt[a], 1] - seg[a, 3])).sum())
    segl = seg.tolist()
    off, pts, _ = chains(S, [None if v < 0 else int(v) for v in nxt], [None if v < 0 else int(v) for v in prv], segl)
    st["paths_out"], st["points_out"] = len(off) - 1, len(pts)
    return off, pts, st


class Doubles:
    """fill_fn and link_fn for orip.stages.fill_strokes and stages/fill_layers.run: the link works on the last fill, as the device's does"""

    def __init__(self):
        self.last, self.fills, self.links = None, 0, 0

    def fill(self, mask, W, H, place, u, spacing, inset, min_len, flags):
        self.last = (np.array(mask), W, H, tuple(place), tuple(u), spacing, inset, min_len, flags)
        self.fills += 1
        return FD.fill_mask(*self.last)

    def link(self, mask, place, reach):
        assert self.last is not None and np.array_equal(mask, self.last[0]) and tuple(place) == self.last[3]      # what the fill was given
        self.links += 1
        return fill_link(*self.last, reach)
