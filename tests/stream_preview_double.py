"""TEST INFRASTRUCTURE: vectorised numpy restatement of the stream preview (csrc/stream_preview.hip, include/orip.h: orip_stream_preview) --
decode, statistics, draw calls and raster -- held to the reference previewer's own statistics and draw-call log
(tests/golden/golden_stream_preview.npz) on the CPU, and to the HIP kernels bit for bit on the GPU.

The raster restates the documented stand-ins for what pygame draws:
  * a 1-px line from pixel p0 to p1: n = max(|dx|, |dy|), pixels p0 + floor((2 j d + n) / (2 n)) for j = 0..n (both ends included);
    at step_scale <= 1 consecutive steps land at most one pixel apart and this is exactly {p0, p1}
  * a tap disc of radius r: every (cx + i, cy + j) with i^2 + j^2 <= r^2
  * pixels outside the clip rect (the workspace, or the surface under --no-clip) are dropped; the last command to draw a pixel sets it."""
import numpy as np

DX = np.array([0, 1, 1, 1, 0, -1, -1, -1], np.int64)
DY = np.array([1, 1, 0, -1, -1, -1, 0, 1], np.int64)
FIELDS = ("total_bytes", "service_bytes", "step_bytes", "single_steps", "double_steps", "steps_total", "pen_down_segments", "taps",
          "color_changes", "speed_changes", "eof_seen", "tail_after_eof", "off_canvas_draws", "final_x", "final_y",
          "unknown_service_bytes", "commands")
# command kinds
K_STEP, K_PEN, K_COLOR, K_SPEED = 0, 1, 2, 3


def geometry(W, H, rw, rh):
    scale = min(rw / max(1, W), rh / max(1, H))
    uw, uh = int(W * scale), int(H * scale)
    return scale, (rw - uw) // 2, (rh - uh) // 2, uw, uh


def decode(data):
    """-> (stats dict without the replay fields, kind[c], val[c]) for the commands in order"""
    b = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    n = len(b)
    eofs = np.flatnonzero(b == 0x3F)
    eof = int(eofs[0]) if len(eofs) else -1
    d = b[:eof + 1] if eof >= 0 else b
    step = (d & 0x80) != 0
    dbl = step & ((d & 0x40) != 0)
    svc = ~step
    pen = svc & ((d == 1) | (d == 2) | (d == 3))
    col = svc & (d >= 8) & (d <= 15)
    spd = svc & ~pen & ~col & (d != 0x3F) & ((d & 0xC0) == 0x40)
    unk = svc & ~pen & ~col & ~spd & (d != 0x3F)
    cnt = np.where(step, np.where(dbl, 2, 1), np.where(pen | col | spd, 1, 0))
    src = np.repeat(np.arange(len(d)), cnt)
    first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    j = np.arange(len(src)) - first[src]
    bs = d[src]
    kind = np.where(step[src], K_STEP, np.where(pen[src], K_PEN, np.where(col[src], K_COLOR, K_SPEED)))
    val = np.where(step[src], np.where(j == 0, (bs >> 3) & 7, bs & 7), np.where(col[src], bs & 7, np.where(spd[src], bs & 0x3F, bs)))
    st = {"total_bytes": n, "service_bytes": int(svc.sum()), "step_bytes": int(step.sum()), "single_steps": int((step & ~dbl).sum()),
          "double_steps": int(dbl.sum()), "steps_total": int((step & ~dbl).sum() + 2 * dbl.sum()), "color_changes": int(col.sum()),
          "speed_changes": int(spd.sum()), "eof_seen": int(eof >= 0), "tail_after_eof": n - (eof + 1) if eof >= 0 else 0,
          "unknown_service_bytes": int(unk.sum()), "commands": int(len(src))}
    return st, kind, val


def _ffill(mask, values, init):
    """value of the last event at or before each index (init before the first)"""
    idx = np.where(mask, np.arange(len(mask)), -1)
    np.maximum.accumulate(idx, out=idx)
    return np.where(idx >= 0, values[np.maximum(idx, 0)], init)


def _to_px(x, y, W, H, scale, ox, oy, invert_y):
    px = np.trunc(ox + x.astype(np.float64) * scale).astype(np.int64)
    yy = (H - 1 - y) if invert_y else y
    py = np.trunc(oy + yy.astype(np.float64) * scale).astype(np.int64)
    return px, py


def replay(data, W, H, rw, rh, invert_y=True, clip=True, render_taps=True, palette=((255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0)), tap_r=5):
    """-> (stats dict in FIELDS order, calls): calls = dict of the draw calls the previewer makes, in order:
    lines int64 [n, 4] (x1, y1, x2, y2), line_ord / line_col (1-based command ordinal, palette index 0..3), circles [m, 3] (cx, cy, r),
    circ_ord / circ_col, plus the clip rect (x, y, w, h) or None"""
    st, kind, val = decode(data)
    c = len(kind)
    isstep = kind == K_STEP
    sdx = np.where(isstep, DX[np.where(isstep, val, 0)], 0)
    sdy = np.where(isstep, DY[np.where(isstep, val, 0)], 0)
    x = np.cumsum(sdx); y = np.cumsum(sdy)                  # position after each command
    x0 = x - sdx; y0 = y - sdy                              # ... and before it
    penev = kind == K_PEN
    down_after = _ffill(penev, (val == 2).astype(np.int64), 0)        # pen state after each command (tap and up lift it)
    down_before = np.concatenate([[0], down_after[:-1]]) if c else down_after
    colidx = _ffill(kind == K_COLOR, val, 0)
    pal = np.minimum(colidx, 3)
    outside = isstep & ~((x >= 0) & (x < W) & (y >= 0) & (y < H))
    st.update({"pen_down_segments": int((penev & (val == 2) & (down_before == 0)).sum()), "taps": int((penev & (val == 3)).sum()),
               "off_canvas_draws": int(outside.sum()), "final_x": int(x[-1]) if c else 0, "final_y": int(y[-1]) if c else 0})
    scale, ox, oy, uw, uh = geometry(W, H, rw, rh)
    ln = np.flatnonzero(isstep & (down_before == 1))
    p0x, p0y = _to_px(x0[ln], y0[ln], W, H, scale, ox, oy, invert_y)
    p1x, p1y = _to_px(x[ln], y[ln], W, H, scale, ox, oy, invert_y)
    tp = np.flatnonzero(penev & (val == 3)) if render_taps else np.zeros(0, np.int64)
    cx, cy = _to_px(x[tp], y[tp], W, H, scale, ox, oy, invert_y)
    calls = {"lines": np.stack([p0x, p0y, p1x, p1y], 1), "line_ord": ln + 1, "line_col": pal[ln],
             "circles": np.stack([cx, cy, np.full(len(tp), tap_r, np.int64)], 1), "circ_ord": tp + 1, "circ_col": pal[tp],
             "clip": (ox, oy, uw, uh) if clip else None, "scale": scale}
    return {k: int(st[k]) for k in FIELDS}, calls


def line_pixels(lines):
    """-> (segment index, px, py) of every pixel of every stand-in line, in call order"""
    L = np.asarray(lines, np.int64).reshape(-1, 4)
    dx, dy = L[:, 2] - L[:, 0], L[:, 3] - L[:, 1]
    n = np.maximum(np.abs(dx), np.abs(dy))
    seg = np.repeat(np.arange(len(L)), n + 1)
    first = np.concatenate([[0], np.cumsum(n + 1)])[:-1]
    j = np.arange(len(seg)) - first[seg]
    nn = np.maximum(n[seg], 1)
    px = L[seg, 0] + (2 * j * dx[seg] + nn) // (2 * nn)
    py = L[seg, 1] + (2 * j * dy[seg] + nn) // (2 * nn)
    return seg, px, py


def disc_offsets(r):
    i, j = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
    m = i * i + j * j <= r * r
    return i[m].astype(np.int64), j[m].astype(np.int64)


def raster_keys(calls, rw, rh):
    """key plane int64 [rh, rw]: 4 * ordinal + palette index of the last command to draw each pixel, 0 = untouched"""
    seg, px, py = line_pixels(calls["lines"])
    key = 4 * calls["line_ord"][seg] + calls["line_col"][seg]
    C = calls["circles"]
    if len(C):
        oi, oj = disc_offsets(int(C[0, 2]))
        px = np.concatenate([px, (C[:, :1] + oi[None]).ravel()]); py = np.concatenate([py, (C[:, 1:2] + oj[None]).ravel()])
        key = np.concatenate([key, np.repeat(4 * calls["circ_ord"] + calls["circ_col"], len(oi))])
    x0, y0, x1, y1 = (0, 0, rw, rh) if calls["clip"] is None else (calls["clip"][0], calls["clip"][1], calls["clip"][0] + calls["clip"][2], calls["clip"][1] + calls["clip"][3])
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, rw), min(y1, rh)
    m = (px >= x0) & (px < x1) & (py >= y0) & (py < y1)
    pix = (py[m] * rw + px[m]); key = key[m]
    out = np.zeros(rw * rh, np.int64)
    if len(pix):
        o = np.argsort(key, kind="stable")                   # in command order: the last occurrence of a pixel is its last writer
        rp, rk = pix[o][::-1], key[o][::-1]
        u, i = np.unique(rp, return_index=True)
        out[u] = rk[i]
    return out.reshape(rh, rw)


def resolve(keys, palette, background_white=True):
    pal = np.asarray(palette, np.uint8).reshape(4, 3)
    bg = np.full(3, 255 if background_white else 0, np.uint8)
    rgb = np.where((keys > 0)[..., None], pal[keys & 3], bg)
    return rgb.astype(np.uint8)


def preview(data, W, H, rw, rh, invert_y=True, clip=True, render_taps=True, background_white=True,
            palette=((255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0)), tap_r=5):
    """the whole preview: (rgb uint8 [rh, rw, 3], stats) for a render surface of rw x rh (already clamped)"""
    st, calls = replay(data, W, H, rw, rh, invert_y, clip, render_taps, palette, tap_r)
    return resolve(raster_keys(calls, rw, rh), palette, background_white), st
