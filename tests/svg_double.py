"""TEST INFRASTRUCTURE: numpy stand-ins for the three device steps of svg2stream (orip_svg_flatten, orip_svg_bbox, orip_svg_fit), so that the host logic of
orip/svg.py can be checked on the CPU and the kernels of csrc/svg.hip against something written independently of them.  The piece count repeats the
device's comparison in IEEE double; the evaluation repeats its order of operations (numpy never fuses); the fit goes through Python's own f"{v:.4f}", which
is what the reference does, and not through the device's residual rule."""
import numpy as np

MAX_PIECES = 1 << 16
MAX_POINTS = (1 << 30) - 1


def transform(table):
    """control points after the segment's raw matrix: x' = (a x + c y) + e, y' = (b x + d y) + f"""
    m = np.asarray(table.raw_mats(), np.float64).reshape(-1, 6)[np.asarray(table.mat, np.int64)]
    c = np.asarray(table.ctrl, np.float64).reshape(-1, 4, 2)
    a, b, cc, d, e, f = (m[:, j, None] for j in range(6))
    x, y = c[:, :, 0], c[:, :, 1]
    with np.errstate(all="ignore"):
        return np.stack([(a * x + cc * y) + e, (b * x + d * y) + f], 2)


def piece_counts(kind, P, tol):
    """the smallest n >= 1 with (n n k)^2 >= w q: k = 4 tol, q the largest squared second difference, w = 1 (quadratic) or 9 (cubic)"""
    kind = np.asarray(kind, np.int64)

    def dd2(a, b, c):
        d = (a - b) + (c - b)
        return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    with np.errstate(all="ignore"):
        q1, q2 = dd2(P[:, 0], P[:, 1], P[:, 2]), dd2(P[:, 1], P[:, 2], P[:, 3])
        wq = np.where(kind == 2, q1, 9.0 * np.maximum(q1, q2))
        wq = np.where(kind <= 1, 0.0, wq)
        if not (np.isfinite(P).all() and np.isfinite(wq).all()):
            raise ValueError("a control point is not finite after its matrix, or the second differences of a curve overflow")
        k = 4.0 * float(tol)
        cand = np.ceil(np.sqrt(np.sqrt(wq) / k))
        n = np.where(cand >= 1.0, np.minimum(cand, MAX_PIECES + 1.0), 1.0).astype(np.int64)

        def enough(n):
            a = (n * n).astype(np.float64) * k
            return a * a >= wq
        while True:
            dec = (n > 1) & enough(np.maximum(n - 1, 1))
            if not dec.any():
                break
            n[dec] -= 1
        while True:
            inc = (n <= MAX_PIECES) & ~enough(n)
            if not inc.any():
                break
            n[inc] += 1
    if (n > MAX_PIECES).any():
        raise ValueError("a curve needs more than 2^16 pieces at this tolerance")
    return n


def _lerp(a, b, t):
    return a + (b - a) * t


def flatten_numpy(table, tol):
    """(off int64 [n_sub + 1], pts float64 [total, 2]) in raw units"""
    if not (tol > 0.0 and np.isfinite(tol)):
        raise ValueError("the tolerance must be a positive finite number")
    kind = np.asarray(table.kind, np.int64); sub_off = np.asarray(table.sub_off, np.int64)
    S, nsub = len(kind), len(sub_off) - 1
    if S == 0:
        return np.zeros(1, np.int64), np.zeros((0, 2))
    if not (np.isfinite(np.asarray(table.ctrl)).all() and np.isfinite(np.asarray(table.mats)).all()):
        raise ValueError("a value is not finite")
    P = transform(table)
    n = piece_counts(kind, P, tol)
    ex = np.concatenate([[0], np.cumsum(n)])
    total = int(ex[-1]) + nsub
    if total > MAX_POINTS:
        raise ValueError("too many points")
    sub_of = np.repeat(np.arange(nsub), np.diff(sub_off))
    first = ex[:-1] + sub_of + 1
    off = np.concatenate([ex[sub_off[:-1]] + np.arange(nsub), [total]]).astype(np.int64)
    out = np.zeros((total, 2))
    out[off[:-1]] = P[sub_off[:-1], 0]
    seg = np.repeat(np.arange(S), n)
    i = np.arange(int(ex[-1])) - ex[:-1][seg] + 1
    t = (i.astype(np.float64) / n[seg].astype(np.float64))[:, None]
    p0, p1, p2, p3 = (P[seg, j] for j in range(4))
    a, b, c = _lerp(p0, p1, t), _lerp(p1, p2, t), _lerp(p2, p3, t)
    u, v = _lerp(a, b, t), _lerp(b, c, t)
    val = np.where((kind[seg] == 2)[:, None], u, _lerp(u, v, t))
    end = P[np.arange(S), np.where(kind <= 1, 1, kind)]
    val = np.where((i == n[seg])[:, None], end[seg], val)
    out[first[seg] + i - 1] = val
    return off, out


def bbox_numpy(paths):
    p = np.asarray(paths[1], np.float64).reshape(-1, 2)
    return float(p[:, 0].min()), float(p[:, 1].min()), float(p[:, 0].max()), float(p[:, 1].max())


def round4_python(v):
    """float(f"{v:.4f}") for every value: what scale_and_offset_gcode writes and a G-code parser reads"""
    flat = np.asarray(v, np.float64).reshape(-1)
    return np.array([float("%.4f" % x) for x in flat.tolist()], np.float64).reshape(np.shape(v))


def fit_numpy(paths, sx, sy, ox, oy):
    off, p = paths
    p = np.asarray(p, np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        x, y = p[:, 0] * float(sx) + float(ox), p[:, 1] * float(sy) + float(oy)
    if len(p) and not ((np.abs(x) < 1e9).all() and (np.abs(y) < 1e9).all()):
        raise ValueError("a fitted coordinate is not finite, or 1e9 and beyond")
    return off, np.stack([round4_python(x), round4_python(y)], 1)


def fetch_numpy(paths, with_points=True):
    return np.asarray(paths[0], np.int64), (np.asarray(paths[1], np.float64).reshape(-1, 2) if with_points else None)


def svg_doubles():
    """the keyword arguments that put every device step of orip.svg.build_stream_from_svg on the CPU"""
    from stream_double import codes_numpy
    import gcode_double as D
    return dict(flatten_fn=flatten_numpy, bbox_fn=bbox_numpy, fit_fn=fit_numpy, fetch_fn=fetch_numpy, steps_fn=lambda paths, m: D.to_steps_numpy(paths[0], paths[1], m),
                order_fn=D.order_numpy, codes_fn=codes_numpy, pack_fn=D.pack_numpy)
