"""TEST INFRASTRUCTURE: small numpy stand-ins for the three device steps of gcode2stream (orip_gcode_to_steps, orip_gcode_order, orip_stream_pack), so that
the host logic of orip/gcode.py can be checked on the CPU against the reference's recorded output.  Written independently of csrc/gcode.hip (no grid, no
piece search: the plain definitions) and themselves pinned by tests/golden/golden_gcode.npz."""
import numpy as np


def to_steps_numpy(off, pts_mm, m):
    off = np.asarray(off, np.int64); p = np.asarray(pts_mm, np.float64).reshape(-1, 2)
    n = len(off) - 1
    if n <= 0 or len(p) == 0:
        return np.zeros(1, np.int64), np.zeros((0, 2), np.int32)
    pid = np.repeat(np.arange(n), np.diff(off))
    with np.errstate(all="ignore"):
        x = (p[:, 0] * m["scale_x"] + m["offset_x_mm"]) * m["steps_per_mm"]
        y = (p[:, 1] * m["scale_y"] + m["offset_y_mm"]) * m["steps_per_mm"]
        if m["invert_y"]:
            y = float(m["H"] - 1) - y
        x, y = np.rint(x), np.rint(y)
    long_enough = (np.diff(off) >= 2)[pid]
    if not (np.isfinite(x) & np.isfinite(y))[long_enough].all():
        raise OverflowError("a coordinate is not finite after the conversion to steps")
    x = np.clip(np.nan_to_num(x), 0, m["W"] - 1).astype(np.int64); y = np.clip(np.nan_to_num(y), 0, m["H"] - 1).astype(np.int64)
    first = np.zeros(len(p), bool); first[off[:-1][np.diff(off) > 0]] = True
    keep = first.copy()
    keep[1:] |= (x[1:] != x[:-1]) | (y[1:] != y[:-1])
    cnt = np.bincount(pid[keep], minlength=n)
    keep &= (cnt >= 2)[pid]
    lens = cnt[cnt >= 2]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.stack([x[keep], y[keep]], 1).astype(np.int32)


def order_numpy(ends):
    """the definition: from (0, 0), the remaining path with the smallest L1 distance to its first point, lowest index on ties; on to its last point"""
    e = np.asarray(ends, np.int64).reshape(-1, 4)
    n = len(e)
    d_dead = np.iinfo(np.int64).max
    alive = np.ones(n, bool)
    out = np.zeros(n, np.int32)
    cx = cy = 0
    for k in range(n):
        d = np.where(alive, np.abs(e[:, 0] - cx) + np.abs(e[:, 1] - cy), d_dead)
        i = int(np.argmin(d))                      # the first minimum: the lowest index
        out[k] = i; alive[i] = False
        cx, cy = e[i, 2], e[i, 3]
    return out


def pack_numpy(table, codes):
    """piece by piece, the way StreamWriter.add_steps pairs the steps of one call"""
    out = bytearray(int(table.nbytes))
    for c0, cnt, pos, spd in zip(table.code0.tolist(), table.cnt.tolist(), table.pos.tolist(), table.speed.tolist()):
        if spd >= 0:
            out[pos] = spd; pos += 1
        c = [int(v) & 7 for v in codes[c0:c0 + cnt]]
        for j in range(0, cnt - 1, 2):
            out[pos] = 0xC0 | (c[j] << 3) | c[j + 1]; pos += 1
        if cnt % 2:
            out[pos] = 0x80 | (c[-1] << 3)
    for p, v in zip(table.svc_pos.tolist(), table.svc_val.tolist()):
        out[p] = v
    return bytes(out)


def order_violations(ends, order, block=512):
    """How many (step k, path chosen later than k) pairs contradict the definition: with the cursor of step k, a later path must have a larger key
    (L1 distance to its first point, index) than the path chosen at k.  Every pair is tested, n^2 / 2 of them, in blocks of `block` steps."""
    e = np.asarray(ends, np.int64).reshape(-1, 4)
    order = np.asarray(order, np.int64)
    n = len(e)
    sx, sy = e[order, 0].astype(np.int32), e[order, 1].astype(np.int32)            # first points in drawing order
    idx = order.astype(np.int32)
    cx = np.concatenate([[0], e[order[:-1], 2]]).astype(np.int32); cy = np.concatenate([[0], e[order[:-1], 3]]).astype(np.int32)   # cursor of every step
    dk = np.abs(cx - sx) + np.abs(cy - sy)
    bad = 0
    for a in range(0, n, block):
        b = min(a + block, n)
        D = np.abs(cx[a:b, None] - sx[None, a:]) + np.abs(cy[a:b, None] - sy[None, a:])
        wrong = (D < dk[a:b, None]) | ((D == dk[a:b, None]) & (idx[None, a:] < idx[a:b, None]))
        wrong[:, :b - a] &= np.triu(np.ones((b - a, b - a), bool), 1)              # only paths chosen LATER than the step
        bad += int(wrong.sum())
    return bad
