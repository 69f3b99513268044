"""Inputs of tests/test_gpu_long_features.py: pairs of long open polylines whose perimeters (numpy's pairwise float32 sum of float32 segment lengths,
O.poly_perimeter) differ by exactly one float32 ulp while a plain left-to-right float32 sum orders them the other way, and that overlap, so that
stage 08's result depends on which of the two ranks first (08-A draws the polylines longest first).  Found by a seeded search; tests/
test_oracle_long_features.py proves every property with the oracle alone."""
import numpy as np

from oracle import oracle as O

CFG6 = dict(O.DEFAULTS, pixels_per_mm=6)          # canvas 1260 x 1782
# point counts: just above ORIP_LONG_POLY (192), 257, one turn of k_poly_features_long (2048 points) + 1, 2048 + ORIP_PF_MARGIN + 1, three turns
SIZES = [193, 194, 257, 2049, 2181, 4300]
CANDIDATES = {193: 6000, 194: 6000, 257: 6000, 2049: 3000, 2181: 3000, 4300: 3000}


def snake(rng, n, x0=40, y0=60, width=1100, pitch=40):
    """n points along rows `width` px long and `pitch` apart, left to right and back: 3 .. 8 px from point to point along the row, up to 2 px off it.
    Two snakes of one size follow the same rows, so they overlap everywhere (collision radius 18 px)."""
    dx = rng.integers(3, 9, n)
    s = np.concatenate([[0], np.cumsum(dx[:-1])])
    row, u = s // width, s % width
    x = np.where(row % 2 == 0, x0 + u, x0 + width - u)
    y = y0 + pitch * row + rng.integers(-2, 3, n)
    return np.stack([x, y], 1).astype(np.int32)


def seglen(p):
    d = (p[1:] - p[:-1]).astype(np.float32)
    return np.sqrt((d * d).sum(1, dtype=np.float32))


def sequential_sum(p):
    return np.cumsum(seglen(p), dtype=np.float32)[-1]


_found = {}


def pair(n):
    """(shorter, longer) by O.poly_perimeter, one ulp apart, the sequential sums the other way round; None when the candidates hold no such pair"""
    if n not in _found:
        rng = np.random.default_rng(n)
        P = [snake(rng, n) for _ in range(CANDIDATES[n])]
        per = np.array([O.poly_perimeter(p) for p in P], np.float32)
        bits = per.view(np.int32)                          # positive floats: consecutive patterns are consecutive values
        order = np.argsort(per, kind="stable")
        _found[n] = None
        for a, b in zip(order[:-1], order[1:]):
            if bits[b] - bits[a] == 1 and sequential_sum(P[a]) > sequential_sum(P[b]):
                _found[n] = (P[a].reshape(-1, 1, 2), P[b].reshape(-1, 1, 2)); break
    return _found[n]


def stage08_in_rank(polys, rank, cfgd=CFG6):
    """O.stage08_layer composed from the oracle's parts, with the drawing order of 08-A given by `rank` (indices into the kept polylines) instead of
    by the perimeters: (lines, taps)"""
    prm = O.derived08(cfgd)
    W, H = O.canvas_size(cfgd)
    kept, taps = O.split_small_taps08(polys, prm)
    assert len(kept) == len(polys)
    forbid = np.zeros((H, W), np.uint8)
    cleaned = []
    for i in rank:
        for seg in O.virtual_draw08(kept[i], forbid, prm):
            parts = O.split_jumps(seg, float(cfgd["max_join_jump_px"]), 8)
            cleaned += parts if parts else [seg]
    lines2, taps2 = O.split_small_taps08(cleaned, prm)
    merged = O.post_skeleton_merge(lines2, prm) if lines2 else lines2
    return O.reorder(merged, 0), taps + taps2


# ---- the resident chain takes no chosen point lists: an image of filled rectangles whose contours, scaled to the canvas, have open views of
# CHAIN_SIZES points (both layers trace the same outlines): 194 and 195 just above ORIP_LONG_POLY, 274, 2066 and 2090 between one turn of
# k_poly_features_long and one turn + ORIP_PF_MARGIN, 2242 beyond it, 4354 in three turns
CHAIN_RECTS = [(10, 10, 12, 14), (10, 40, 14, 22), (10, 80, 16, 30), (40, 10, 40, 60), (10, 180, 20, 40), (10, 240, 24, 40), (100, 10, 110, 150),
               (100, 180, 120, 162), (100, 360, 112, 151), (240, 10, 174, 372), (40, 90, 42, 70)]           # (y, x, height, width)
CHAIN_SIZES = {194, 195, 274, 2066, 2090, 2242, 4354}


def chain_image():
    img = np.full((430, 540, 3), 235, np.uint8)
    for y, x, h, w in CHAIN_RECTS:
        img[y:y + h, x:x + w] = 30
    return img


def chain_cfg():
    from orip.synth import layer_names
    return dict(O.DEFAULTS, color_names=layer_names(2), pixels_per_mm=6)


def open_view_sizes(polys):
    out = []
    for p in polys:
        a = np.asarray(p).reshape(-1, 2)
        out.append(len(a) - (1 if len(a) >= 2 and (a[0] == a[-1]).all() else 0))
    return out
