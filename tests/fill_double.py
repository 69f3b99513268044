"""Sequential double of orip_fill_mask (include/orip.h states the rule): plain Python integers, one loop over k and one over a for every family.
Nothing in fill_mask is vectorised or clever on purpose: it is the text of the rule, to be compared by equality.  fill_mask_numpy, at the end, is the same
rule over arrays for the large inputs of tests/hatch_scale_cases.py, and is held to fill_mask by equality."""
import math

import numpy as np

SERPENTINE, ALONG, ACROSS = 1, 2, 4
STATS = ("lines", "samples", "on", "runs", "short", "segments")


def rs(v: int) -> int:
    return (math.isqrt(4 * v) + 1) >> 1


def frame(u, spacing: int, inset: int, min_len: int):
    """(R, D, m, im, lm) of a direction"""
    ux, uy = int(u[0]), int(u[1])
    U2 = ux * ux + uy * uy
    R, D, m = rs(U2), rs(spacing * spacing * U2), max(abs(ux), abs(uy))
    return R, D, m, (2 * inset * m + R) // (2 * R), max(1, (2 * min_len * m + R) // (2 * R))


def sample(u, D: int, W: int, H: int, k: int, a: int):
    """canvas pixel (X, Y) of sample (k, a), or None when it does not exist"""
    ux, uy = u
    xmajor = abs(ux) >= abs(uy)
    N, d = (k * D + uy * a, ux) if xmajor else (ux * a - k * D, uy)
    if d < 0:
        N, d = -N, -d
    b = (2 * N + d) // (2 * d)
    if not 0 <= b < (H if xmajor else W):
        return None
    return (a, b) if xmajor else (b, a)


def ink(M, place, X: int, Y: int) -> bool:
    num, den, dx, dy = place
    c, r = ((X - dx) * den) // num, ((Y - dy) * den) // num
    return 0 <= c < M.shape[1] and 0 <= r < M.shape[0] and M[r, c] != 0


def fill_mask(mask, W, H, place, u, spacing, inset, min_len, flags):
    """-> (seg int32 [segments, 4], {STATS})"""
    M = np.asarray(mask)
    place = tuple(int(v) for v in place)
    st = dict.fromkeys(STATS, 0)
    segs = []
    fams = ([(int(u[0]), int(u[1]))] if flags & ALONG else []) + ([(-int(u[1]), int(u[0]))] if flags & ACROSS else [])
    assert fams and not flags & ~7
    for f in fams:
        R, D, m, im, lm = frame(f, spacing, inset, min_len)
        xmajor = abs(f[0]) >= abs(f[1])
        A = W if xmajor else H
        corners = [-f[1] * x + f[0] * y for x in (0, W - 1) for y in (0, H - 1)]
        for k in range((min(corners) - m) // D - 1, (max(corners) + m) // D + 2):       # wider than any line with a sample: |n.P - k D| <= m / 2
            on, exists = [], 0
            for a in range(A):
                P = sample(f, D, W, H, k, a)
                exists += P is not None
                on.append(P is not None and ink(M, place, *P))
            if not exists:
                continue
            st["lines"] += 1; st["samples"] += exists; st["on"] += sum(on)
            line, a = [], 0
            while a < A:
                if not on[a]:
                    a += 1
                    continue
                a0 = a
                while a + 1 < A and on[a + 1]:
                    a += 1
                a1 = a
                a += 1
                st["runs"] += 1
                s0, s1 = a0 + im, a1 - im
                if s1 - s0 >= lm:
                    line.append(sample(f, D, W, H, k, s0) + sample(f, D, W, H, k, s1))
                else:
                    st["short"] += 1
            if flags & SERPENTINE and k & 1:
                line = [(x1, y1, x0, y0) for x0, y0, x1, y1 in reversed(line)]
            st["segments"] += len(line)
            segs += line
    return np.asarray(segs, np.int32).reshape(-1, 4), st


def fill_mask_numpy(mask, W, H, place, u, spacing, inset, min_len, flags, lines_at_once=None):
    """fill_mask once more, as int64 arrays over (k, a): the same rule, the same pair (segments, stats), for the inputs of millions of samples that the loops
    above cannot afford.  It is pinned to fill_mask by equality on every case of tests/fill_cases.py (test_hatch_scale_host.py).  The lines are taken
    `lines_at_once` at a time (default: about 2^21 samples), which bounds the memory and changes nothing."""
    M = np.asarray(mask) != 0
    num, den, dx, dy = (int(v) for v in place)
    st = dict.fromkeys(STATS, 0)
    out = []
    fams = ([(int(u[0]), int(u[1]))] if flags & ALONG else []) + ([(-int(u[1]), int(u[0]))] if flags & ACROSS else [])
    assert fams and not flags & ~7
    for ux, uy in fams:
        R, D, m, im, lm = frame((ux, uy), spacing, inset, min_len)
        xmajor = abs(ux) >= abs(uy)
        A, B = (W, H) if xmajor else (H, W)
        d = ux if xmajor else uy

        def minor(k, a):                                                              # b of sample (k, a), arrays
            N = k * D + uy * a if xmajor else ux * a - k * D
            return (2 * N + d) // (2 * d) if d > 0 else (-2 * N - d) // (-2 * d)

        corners = [-uy * x + ux * y for x in (0, W - 1) for y in (0, H - 1)]
        k_lo, k_hi = (min(corners) - m) // D - 1, (max(corners) + m) // D + 2
        step = lines_at_once or max(1, (1 << 21) // A)
        a = np.arange(A, dtype=np.int64)[None, :]
        for k0 in range(k_lo, k_hi, step):
            k = np.arange(k0, min(k0 + step, k_hi), dtype=np.int64)[:, None]
            b = minor(k, a)
            ex = (b >= 0) & (b < B)
            X, Y = (np.broadcast_to(a, b.shape), b) if xmajor else (b, np.broadcast_to(a, b.shape))
            c, r = ((X - dx) * den) // num, ((Y - dy) * den) // num
            ok = ex & (c >= 0) & (c < M.shape[1]) & (r >= 0) & (r < M.shape[0])
            on = np.zeros(b.shape, bool)
            on[ok] = M[r[ok], c[ok]]
            st["lines"] += int(ex.any(1).sum()); st["samples"] += int(ex.sum()); st["on"] += int(on.sum())
            e = np.diff(np.pad(on.astype(np.int8), ((0, 0), (1, 1))), axis=1)         # +1 in front of a run's first sample, -1 behind its last
            l0, a0 = np.nonzero(e == 1)
            l1, a1 = np.nonzero(e == -1)                                              # row-major, so the i-th start and the i-th end are one run
            assert np.array_equal(l0, l1)
            s0, s1 = a0 + im, a1 - 1 - im
            keep = s1 - s0 >= lm
            st["runs"] += len(a0); st["short"] += int((~keep).sum()); st["segments"] += int(keep.sum())
            kk, s0, s1 = k[l0[keep], 0], s0[keep], s1[keep]
            b0, b1 = minor(kk, s0), minor(kk, s1)
            assert ((b0 >= 0) & (b0 < B) & (b1 >= 0) & (b1 < B)).all()
            seg = np.stack([s0, b0, s1, b1] if xmajor else [b0, s0, b1, s1], 1)
            if flags & SERPENTINE:
                back = (kk & 1) == 1
                seg[back] = seg[back][:, [2, 3, 0, 1]]
                seg = seg[np.lexsort((np.where(back, -s0, s0), kk))]
            out.append(seg)
    seg = np.concatenate(out) if out else np.zeros((0, 4), np.int64)
    return seg.astype(np.int32).reshape(-1, 4), st
