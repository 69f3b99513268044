"""The sequential double of orip_fill_stipple (include/orip.h states the rule): Python integers, every candidate and every window pixel visited one after
the other, nothing vectorised.  It is the statement of the rule the GPU tests compare against, by equality.

Beside it closed_form(): numpy, for clear_rad = tone_rad = 0 only.  There the clearance is the centre pixel itself, C = 1 and S = G[r, c], so the rule is one
expression per lattice point; tests/test_fill_stipple_host.py shows it equal to the double on every small case with those radii, and it gives the case past
the launch caps its expected answer in seconds."""
import numpy as np

STATS = ("candidates", "ink", "near", "light", "dots")
SERPENTINE = 1


def bayer(i, j):
    """T of lattice point (i, j): the 8 x 8 Bayer matrix"""
    x, y = i & 7, j & 7
    v = x ^ y
    return ((v & 1) << 5) | ((y & 1) << 4) | ((v & 2) << 2) | ((y & 2) << 1) | ((v & 4) >> 1) | ((y & 4) >> 2)


def fill_stipple(mask, tone, W, H, place, lattice, clear_rad, tone_rad, lo, hi, flags):
    """-> (xy int32 [dots, 2], {STATS}); the arguments of orip.device.Device.fill_stipple"""
    M = np.asarray(mask, np.uint8)
    h, w = M.shape
    G = (np.zeros((h, w), np.uint8) if tone is None else np.asarray(tone, np.uint8)).tolist()
    M = M.tolist()
    num, den, dx, dy = (int(v) for v in place)
    pitch, row, shift = (int(v) for v in lattice)
    R = hi - lo
    st = dict.fromkeys(STATS, 0)
    out = []
    j = 0
    while j * row < H:
        Y = j * row
        line = []
        i = 0
        while i * pitch + (shift if j & 1 else 0) < W:
            X = i * pitch + (shift if j & 1 else 0)
            st["candidates"] += 1
            c, r = (X - dx) * den // num, (Y - dy) * den // num                        # Python's // is the floor division
            if 0 <= c < w and 0 <= r < h and M[r][c] != 0:
                st["ink"] += 1
                clear = True
                for rr in range(r - clear_rad, r + clear_rad + 1):
                    for cc in range(c - clear_rad, c + clear_rad + 1):
                        if not (0 <= rr < h and 0 <= cc < w and M[rr][cc] != 0):
                            clear = False
                if not clear:
                    st["near"] += 1
                else:
                    C = S = 0
                    for rr in range(max(r - tone_rad, 0), min(r + tone_rad, h - 1) + 1):
                        for cc in range(max(c - tone_rad, 0), min(c + tone_rad, w - 1) + 1):
                            if M[rr][cc] != 0:
                                C += 1
                                S += G[rr][cc]
                    E = min(max(255 * C - S - lo * C, 0), R * C)
                    if 64 * E > bayer(i, j) * R * C:
                        st["dots"] += 1
                        line.append((X, Y))
                    else:
                        st["light"] += 1
            i += 1
        out += reversed(line) if (flags & SERPENTINE) and (j & 1) else line
        j += 1
    return np.asarray(out, np.int32).reshape(-1, 2), st


def closed_form(mask, tone, W, H, place, lattice, clear_rad, tone_rad, lo, hi, flags):
    """the same answer for clear_rad = tone_rad = 0, one expression per lattice point"""
    assert clear_rad == 0 and tone_rad == 0
    M = np.asarray(mask, np.uint8)
    h, w = M.shape
    G = np.zeros((h, w), np.int64) if tone is None else np.asarray(tone, np.int64)
    num, den, dx, dy = (int(v) for v in place)
    pitch, row, shift = (int(v) for v in lattice)
    j = np.arange((H - 1) // row + 1, dtype=np.int64)[:, None]
    i = np.arange((W - 1) // pitch + 1, dtype=np.int64)[None, :]
    X, Y = i * pitch + np.where(j & 1, shift, 0), j * row + 0 * i
    cand = X < W
    c, r = (X - dx) * den // num, (Y - dy) * den // num
    inside = cand & (c >= 0) & (c < w) & (r >= 0) & (r < h)
    cs, rs = np.clip(c, 0, w - 1), np.clip(r, 0, h - 1)
    ink = inside & (M[rs, cs] != 0)
    E = np.clip(255 - G[rs, cs] - lo, 0, hi - lo)
    x, y = i & 7, j & 7
    v = x ^ y
    T = ((v & 1) << 5) | ((y & 1) << 4) | ((v & 2) << 2) | ((y & 2) << 1) | ((v & 4) >> 1) | ((y & 4) >> 2)
    dot = ink & (64 * E > T * (hi - lo))
    rows = []
    for jj in range(dot.shape[0]):
        xs = X[jj][dot[jj]]
        if (flags & SERPENTINE) and (jj & 1):
            xs = xs[::-1]
        rows.append(np.stack([xs, np.full(len(xs), jj * row, np.int64)], 1))
    xy = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 2), np.int32)
    n = int(dot.sum())
    return xy.reshape(-1, 2), dict(candidates=int(cand.sum()), ink=int(ink.sum()), near=0, light=int(ink.sum()) - n, dots=n)
