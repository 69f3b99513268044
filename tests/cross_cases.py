"""Inputs for stage 10 (csrc/vector10.hip, the cross-layer dedup) at its edges, shared by test_oracle_cross_cases.py (no GPU: shows with the oracle's parts and a
numpy restatement of the kernels' branch conditions that every case reaches what its name says, and pins hand-worked answers) and test_gpu_cross_cases.py (runs
them on the device through the ABI struct and compares with the oracle, exactly).  Plain data and numpy: the functions that need the oracle take it as `O`.

A case is a dict: name, W, H, prm (the fields of orip_params10 that differ from BASE), layers (a list of (lines, taps), dark -> light).

Two devices keep the cases exact and small.
  * D_lines = 1 gives a line brush of radius 0: a layer paints exactly the vertices of its own kept lines.  A kept line has at least two points, so the smallest
    thing a darker layer can forbid is a `domino` of two neighbouring pixels; the cases put the second pixel where the layer under test never looks.
  * probes: one polyline per canvas row (column), from end to end, in the layer after the one that paints, with a vertex on every pixel (the step points of a
    two-point polyline are (W - 1) * float32(k / (W - 1)), which is not a whole number for every k and W).  The cut then tests every pixel; with
    min_keep = 0 and tap_diam = 0 every piece is kept and none becomes a tap, so the surviving runs are the free pixels.  A run of one point is dropped, so a free
    pixel that has no free neighbour in its row shows only under the column probes and the other way round; one that is alone in both directions shows in neither.
    The paint cases are chosen so that the oracle's raster has no such pixel (asserted on the CPU)."""
import math

import numpy as np

import param_cases

FIELDS = ["tap_diam", "min_keep", "tap_max_per", "tap_max_v", "max_jump", "D_lines", "D_taps", "step_px", "W", "H"]
# nothing is a tap (2 r >= 2e-4 > 0), everything is kept, line brush radius 0, tap brush radius 1
BASE = dict(tap_diam=0.0, min_keep=0.0, tap_max_per=150.0, tap_max_v=50, max_jump=80.0, D_lines=1.0, D_taps=2.0, step_px=1.0)
NAMES = ["layer_dark", "layer_mid", "layer_skin", "layer_light"]          # oracle.darkness_rank10 keeps this order
F = np.float32


def P(a):
    return np.asarray(a, np.int32).reshape(-1, 1, 2)


def case(name, W, H, layers, **prm):
    assert len(layers) <= len(NAMES)
    return dict(name=name, W=W, H=H, prm=prm, layers=layers)


def prm_of(c, **over):
    return dict(BASE, W=c["W"], H=c["H"], **dict(c["prm"], **over))


def prm_vec(p):
    return np.array([p[k] for k in FIELDS], np.float64)


def rad_lines(p):
    return int(max(1, int(np.rint(p["D_lines"])))) // 2          # np.rint rounds half to even, as the stage does


def rad_taps(p):
    return int(max(1, int(np.rint(p["D_taps"] / 2.0))))


def want(O, c, **over):
    """the oracle's answer for the case: [(lines, taps)] per layer"""
    names = NAMES[:len(c["layers"])]
    cfgd = dict(pixels_per_mm=1, target_width_mm=c["W"], target_height_mm=c["H"], color_names=names)
    out = param_cases.stage10_with(O, dict(zip(names, c["layers"])), cfgd, prm_vec(prm_of(c, **over)))
    return [out[n] for n in names]


def raster_after(O, c, n_layers, **over):
    """(results, forbidden raster) after the first n_layers layers"""
    forb = np.zeros((c["H"], c["W"]), np.uint8); res = []
    for lines, taps in c["layers"][:n_layers]:
        res.append(O.stage10_layer(lines, taps, forb, prm_vec(prm_of(c, **over))))
    return res, forb


# ---------------------------------------------------------------- the kernels' conditions, restated
def step_points(poly, step=1.0):
    """k_cut_counts / k_cut_slots: the float32 step points of a polyline, [m, 2] float32 (before the raster test and the truncation)"""
    xy = np.asarray(poly).reshape(-1, 2)
    if len(xy) < 2:
        return np.zeros((0, 2), F)
    out = [(F(xy[0, 0]), F(xy[0, 1]))]
    for i in range(1, len(xy)):
        p0x, p0y = F(xy[i - 1, 0]), F(xy[i - 1, 1])
        vx, vy = F(F(xy[i, 0]) - p0x), F(F(xy[i, 1]) - p0y)
        L = float(F(math.sqrt(float(vx) * float(vx) + float(vy) * float(vy))))
        if L <= 1e-6:
            continue
        nn = max(1, int(math.ceil(L / max(1.0, step))))
        t = (np.arange(1, nn + 1, dtype=np.float64) / float(nn)).astype(F)
        qx = p0x + vx * t; qy = p0y + vy * t          # float32 throughout
        out += list(zip(qx, qy))
    return np.array(out, F).reshape(-1, 2)


def slot_counts(poly):
    """cnt[] of k_cut_counts for one polyline"""
    xy = np.asarray(poly).reshape(-1, 2).astype(np.float64)
    if len(xy) < 2:
        return [0] * len(xy)
    L = np.sqrt(((xy[1:] - xy[:-1]) ** 2).sum(1))
    return [1] + [int(max(1, math.ceil(l))) if l > 1e-6 else 0 for l in L]


def branch_of(piece, p):
    """k_tiny_taps10 for one cut piece: which of its three branches is taken.  'big': the bbox alone says keep; 'many': too many vertices for a tap and
    the bbox says not tiny; 'circle': the enclosing circle is computed"""
    xy = np.asarray(piece).reshape(-1, 2)
    ext = float(max(xy[:, 0].max() - xy[:, 0].min(), xy[:, 1].max() - xy[:, 1].min()))
    if ext > max(p["tap_diam"], p["min_keep"]) + 2.0:
        return "big"
    if len(xy) > p["tap_max_v"] and ext >= p["min_keep"] + 2.0:
        return "many"
    return "circle"


def fate_of(O, piece, p):
    """'tap' / 'keep' / 'drop' by the kernel's conditions, with the oracle's circle and arc length"""
    b = branch_of(piece, p)
    if b != "circle":
        return "keep"
    xy = np.asarray(piece).reshape(-1, 2)
    d = 2.0 * float(F(O.min_enclosing_circle(xy.astype(F))[1]))
    if d <= p["tap_diam"] and len(xy) <= p["tap_max_v"] and O.arc_length(piece, False) <= p["tap_max_per"]:
        return "tap"
    return "keep" if d >= p["min_keep"] else "drop"


def diameter(O, piece):
    return 2.0 * float(F(O.min_enclosing_circle(np.asarray(piece).reshape(-1, 2).astype(F))[1]))


# cv::minEnclosingCircle in float32 as mec_wave runs it: three nested searches for the next point outside the current circle, 64 candidates at a time.  Every find is
# recorded as (level, chunks advanced since the search last restarted, lane): (.., 0, 63) is the last lane of a chunk, (.., 1, 0) the first lane of the next one.
_EPS = F(1.0e-4)


def _nrm(dx, dy):
    return math.sqrt(float(dx) * float(dx) + float(dy) * float(dy))


def _circle3(a, b, c):
    v1 = (F(b[0] - a[0]), F(b[1] - a[1])); v2 = (F(c[0] - a[0]), F(c[1] - a[1]))
    m1 = (F(F(a[0] + b[0]) / F(2)), F(F(a[1] + b[1]) / F(2))); c1 = F(F(m1[0] * v1[0]) + F(m1[1] * v1[1]))
    m2 = (F(F(a[0] + c[0]) / F(2)), F(F(a[1] + c[1]) / F(2))); c2 = F(F(m2[0] * v2[0]) + F(m2[1] * v2[1]))
    det = F(F(v1[0] * v2[1]) - F(v1[1] * v2[0]))
    if abs(det) <= _EPS:
        sq = lambda p, q: F(F(F(p[0] - q[0]) * F(p[0] - q[0])) + F(F(p[1] - q[1]) * F(p[1] - q[1])))
        d1, d2, d3 = sq(a, b), sq(a, c), sq(b, c)
        r = F(F(np.sqrt(max(d1, d2, d3)) * F(0.5)) + _EPS)
        if d1 >= d2 and d1 >= d3: p, q = a, b
        elif d2 >= d1 and d2 >= d3: p, q = a, c
        else: p, q = b, c
        return (F(F(p[0] + q[0]) * F(0.5)), F(F(p[1] + q[1]) * F(0.5))), r
    cx = F(F(F(c1 * v2[1]) - F(c2 * v1[1])) / det); cy = F(F(F(v1[0] * c2) - F(v2[0] * c1)) / det)
    ex, ey = F(cx - a[0]), F(cy - a[1])
    return (cx, cy), F(np.sqrt(F(F(ex * ex) + F(ey * ey))) + _EPS)


def _diam(a, b):
    return (F(F(a[0] + b[0]) / F(2)), F(F(a[1] + b[1]) / F(2))), F(F(F(_nrm(F(a[0] - b[0]), F(a[1] - b[1]))) / F(2)) + _EPS)


def mec_trace(points, drop=None):
    """((cx, cy), r, finds) for n >= 3 points.  drop = (level, chunks, lane): the search overlooks what it would find there (what a wrong chunk advance or a lost
    lane does) -- a case built for that place must then end with another circle"""
    pts = [(F(x), F(y)) for x, y in np.asarray(points).reshape(-1, 2)]
    finds = []

    def lost(level, k, k0):
        return drop is not None and drop[0] == level and (k - k0) // 64 == drop[1] and drop[2] in (None, (k - k0) % 64)

    def third(i, j):
        c, r = _diam(pts[j], pts[i]); k0 = 0
        for k in range(j):
            if _nrm(F(c[0] - pts[k][0]), F(c[1] - pts[k][1])) < float(r):
                continue
            if lost("inner", k, k0):
                continue
            finds.append(("inner", (k - k0) // 64, (k - k0) % 64)); k0 = k + 1
            nc, nr = _circle3(pts[i], pts[j], pts[k])
            if nr > 0: c, r = nc, nr
        return c, r

    def second(i):
        c, r = _diam(pts[0], pts[i]); j0 = 1
        for j in range(1, i):
            if _nrm(F(c[0] - pts[j][0]), F(c[1] - pts[j][1])) < float(r):
                continue
            if lost("middle", j, j0):
                continue
            finds.append(("middle", (j - j0) // 64, (j - j0) % 64)); j0 = j + 1
            nc, nr = third(i, j)
            if nr > 0: c, r = nc, nr
        return c, r

    c, r = _diam(pts[0], pts[1]); i0 = 2
    for i in range(2, len(pts)):
        if F(_nrm(F(pts[i][0] - c[0]), F(pts[i][1] - c[1]))) < r:
            continue
        if lost("outer", i, i0):
            continue
        finds.append(("outer", (i - i0) // 64, (i - i0) % 64)); i0 = i + 1
        nc, nr = second(i)
        if nr > 0: c, r = nc, nr
    return (float(c[0]), float(c[1])), float(r), finds


def bits(x):
    return int(np.array(x, F).view(np.uint32))


# ---------------------------------------------------------------- builders
def domino(x, y, dx=1, dy=0):
    """forbids pixels (x, y) and (x + dx, y + dy) under a line brush of radius 0"""
    return P([[x, y], [x + dx, y + dy]])


def walk(pts):
    """a polyline whose consecutive vertices are one axis step apart: the 1-px resample of the cut returns it vertex by vertex"""
    a = np.asarray(pts, np.int64).reshape(-1, 2)
    assert (np.abs(np.diff(a, axis=0)).sum(1) == 1).all()
    return P(a)


def manhattan(a, b):
    """unit steps from a to b (a excluded, b included): x first, then y"""
    out = []; x, y = a
    while x != b[0]:
        x += 1 if b[0] > x else -1; out.append((x, y))
    while y != b[1]:
        y += 1 if b[1] > y else -1; out.append((x, y))
    return out


def snake(n, x0, y0, row=100):
    """n vertices 1 px apart: rows of `row` pixels, there and back"""
    pts = []; x, y, d = x0, y0, 1
    while len(pts) < n:
        pts.append((x, y))
        if len(pts) % row == 0:
            y += 1; d = -d
        else:
            x += d
    return walk(pts)


# ---------------------------------------------------------------- A. cut
def _cut_cases():
    out = {}
    # Unit diagonals: the step points between the vertices are (10.5, 10.5), (11.5, 11.5), ...  Pixel (11, 11) is forbidden (its domino partner (12, 11) is off the
    # diagonal).  The raster is read at round-half-even, the point is emitted truncated:
    #   (10.5, 10.5) reads (10, 10) free     [half-up would read (11, 11)]          (11.5, 11.5) reads (12, 12) free     [truncation would read (11, 11)]
    out["rounding_triple"] = case("rounding_triple", 40, 30, [([domino(11, 11)], []), ([P([[10, 10], [11, 11], [12, 12], [13, 13], [14, 14]])], [])])
    # fractional step points left of x = 0 and above y = 0: (-0.6) reads pixel -1 (outside, never blocked) and is emitted as 0
    out["across_zero"] = case("across_zero", 40, 30, [([domino(0, 0), domino(0, 3, 0, 1), domino(3, 0), domino(2, 2)], []),
                                                       ([P([[-3, -2], [4, 3]]), P([[-2, 5], [3, -3]]), P([[-5, 0], [6, 1]]), P([[1, -4], [0, 7]]), P([[-1, -1], [-1, 6]]), P([[-4, -1], [5, -1]])], [])])
    out["beyond_far_edges"] = case("beyond_far_edges", 40, 30, [([domino(38, 29), domino(39, 26, 0, 1), domino(36, 28)], []),
                                                                 ([P([[33, 24], [45, 33]]), P([[35, 35], [43, 22]]), P([[30, 29], [50, 30]]), P([[39, 20], [40, 36]]), P([[40, 20], [40, 33]]), P([[30, 30], [44, 30]])], [])])
    # zero-length segments: count 0, and the slot's owner is searched backwards over them
    out["repeated_vertices"] = case("repeated_vertices", 40, 30, [([domino(8, 12, 0, 1)], []),
                                                                  ([P([[5, 5], [5, 5], [9, 5]]), P([[5, 8], [7, 8], [7, 8], [7, 8], [9, 10]]), P([[5, 12], [9, 12], [9, 12]]), P([[20, 20]] * 4),
                                                                    P([[5, 15], [5, 15], [5, 15], [6, 15], [6, 15]])], [])])
    out["one_point_polylines"] = case("one_point_polylines", 40, 30, [([P([[3, 3]]), domino(6, 6), P([[7, 7]])], []),
                                                                      ([P([[1, 1]]), P([[2, 6], [9, 6]]), P([[6, 6]]), P([[30, 2]]), P([[2, 8], [9, 8]]), P([[9, 9]])], []),
                                                                      ([P([[4, 4]]), P([[5, 5]])], [])])
    # y = 20, x = 10 .. 30: forbidden at the first point, the last point, x = 13 (leaves the run 11, 12) and x = 15 (leaves the run 14 alone)
    out["ends_and_short_runs"] = case("ends_and_short_runs", 40, 30, [([domino(x, 20, 0, 1) for x in (10, 13, 15, 30)], []), ([P([[10, 20], [30, 20]])], [])])
    # more than 256 vertices in one polyline: the threads of a block come round again.  Vertex i of the 257- and the 600-vertex snake is forbidden for i = 255, 256
    # (and 511, 512): the last thread of one round and the first of the next.  Two neighbouring vertices are one domino
    def snakes(n, y0):
        s = snake(n, 5, y0); v = s.reshape(-1, 2)
        if n == 256:
            return s, [domino(int(v[255, 0]), int(v[255, 1]), 0, 1)]          # (the row below the snake is empty)
        return s, [P([v[i], v[i + 1]]) for i in (255, 511) if i + 1 < n]
    blk = []; ln = []
    for n, y0 in ((256, 2), (257, 6), (600, 10)):
        s, b = snakes(n, y0); ln.append(s); blk += b
    out["long_polylines"] = case("long_polylines", 120, 40, [(blk, []), (ln, [])])
    # one segment of ~45 000 steps with float32 products to round; it crosses the canvas, where a few pixels are forbidden
    obl = [P([[-16000, -15990], [16001, 15987]]), P([[15990, -11037], [-15800, 11200]])]
    blk = []
    for p in obl:          # forbid pairs of pixels the line itself reads, a quarter, a half and three quarters of its way through the canvas
        px = np.rint(step_points(p)).astype(np.int64); px = px[(px[:, 0] >= 0) & (px[:, 0] < 200) & (px[:, 1] >= 0) & (px[:, 1] < 140)]
        blk += [P([px[k], px[k + 1]]) for k in (len(px) // 4, len(px) // 2, 3 * len(px) // 4)]
    out["long_oblique"] = case("long_oblique", 200, 140, [(blk, []), (obl, [])])
    return out


CUT = _cut_cases()
# hand-worked answers of the last layer: the pieces in travel order (the longest first, then the nearest end, flipped when its far end is nearer)
CUT_LITERAL = {
    "rounding_triple": [[(11, 11), (12, 12), (12, 12), (13, 13), (13, 13), (14, 14)], [(10, 10), (10, 10)]],
    "ends_and_short_runs": [[(x, 20) for x in range(16, 30)], [(12, 20), (11, 20)]],
}
# what the other two rounding rules would give on rounding_triple (before the travel order)
TRIPLE_HALF_UP = [[(11, 11), (12, 12), (12, 12), (13, 13), (13, 13), (14, 14)]]
TRIPLE_TRUNC = [[(10, 10), (10, 10)], [(12, 12), (12, 12), (13, 13), (13, 13), (14, 14)]]

# the large layer: more polylines than the grids of k_cut_counts / k_tiny_taps10 have blocks, every one a tap, more tap candidates than the one-wave filter
# takes, more accepted taps than the 1024 threads of the other one
LARGE_N = 65536 + 300
LARGE_SPOTS = 2600          # distinct tap positions; the last 300 polylines bring positions of their own


def large_case():
    n_old = LARGE_N - 300
    k = np.arange(LARGE_N); spot = np.where(k < n_old, k % (LARGE_SPOTS - 300), LARGE_SPOTS - 300 + (k - n_old))
    x = 10 + 6 * (spot % 300); y = 10 + 4 * (spot // 300)
    a = np.stack([x, y, x + 3, y], 1).astype(np.int32).reshape(-1, 2, 1, 2)
    return case("large_layer", 2000, 2000, [(list(a), [])], tap_diam=4.0, min_keep=0.0)


# ---------------------------------------------------------------- B. tiny and the tap rule
B_PRM = dict(tap_diam=100.0, min_keep=40.0, tap_max_v=1000, tap_max_per=1.0e6)          # boxes up to 42 px reach the circle; every piece is a tap


def _osc(n, a=(0, 0), b=(1, 0)):
    return [a if k % 2 == 0 else b for k in range(n)]


def _tiny_pieces():
    o = (20, 20)
    sh = lambda pts: [(x + o[0], y + o[1]) for x, y in pts]
    out = {}
    # point counts around the 64-wide searches (the cut returns a unit walk as it is)
    for n in (2, 3, 63, 64, 65, 66, 127, 128, 129, 200):
        out["count_%d" % n] = walk(sh(snake(n, 0, 0, row=12).reshape(-1, 2)))
    # three-point shapes: the vertices are 4 .. 9 px apart, the piece is their 1-px resample
    out["three_acute"] = P(sh([(0, 0), (8, 1), (3, 7)]))
    out["three_right"] = P(sh([(0, 0), (6, 0), (6, 8)]))
    out["three_obtuse"] = P(sh([(0, 0), (4, 1), (9, 0)]))
    out["three_collinear"] = P(sh([(0, 0), (3, 0), (7, 0)]))
    out["three_collinear_diagonal"] = P(sh([(0, 0), (2, 2), (5, 5)]))
    # duplicated points: a diagonal unit step is cut into (x, y), (x, y), (x + 1, y + 1); a walk that comes back repeats points further apart
    out["duplicates_diagonal"] = P(sh([(0, 0), (1, 1), (2, 2), (3, 1), (4, 0), (3, 1)]))
    out["duplicates_first_two"] = P(sh([(0, 0), (1, 1), (5, 3)]))
    out["duplicates_revisit"] = walk(sh([(0, 0), (1, 0), (2, 0), (1, 0), (0, 0), (0, 1), (0, 0), (1, 0), (2, 0), (3, 0)]))
    # where the searches find their first point outside (VIOLATOR_WALKS)
    for name, pts in VIOLATOR_WALKS.items():
        out[name] = walk(sh(pts))
    return out


# unit walks that put a find of each search at a chosen place (test_oracle_cross_cases.py asserts what each reaches, with mec_trace)
VIOLATOR_WALKS = {}


def _fill_violator_walks():
    for tag, a in (("lane63", 64), ("next_lane0", 65), ("deep", 1 + 64 * 2 + 9)):
        # middle: the point at index a is the first one outside the circle over point 0 and the point that ends the walk.  A unit walk alternates between the two
        # colours of the chessboard, so an odd and an even index need different points
        if a % 2:          # ... (0, 0) | (0, 1) (1, 1) (1, 0) (2, 0): the circle over (0, 0) - (2, 0) holds (1, 0) and (1, 1), not (0, 1)
            VIOLATOR_WALKS["middle_" + tag] = _osc(a) + [(0, 1), (1, 1), (1, 0), (2, 0)]
        else:              # ... (1, 0) (2, 0) (2, 1) | (2, 2) (2, 1) (2, 0) (3, 0): the circle over (0, 0) - (3, 0) holds (2, 1), not (2, 2)
            VIOLATOR_WALKS["middle_" + tag] = _osc(a - 2) + [(2, 0), (2, 1), (2, 2), (2, 1), (2, 0), (3, 0)]
    # inner: the first a points stay on (0, 0) / (1, 0); the tails were found by trying random walks until one of the circles over two later points holds all of
    # the first a points, not the next one, and the walk ends with another circle when that find is overlooked
    for tag, a, tail in (("lane63", 63, [(1, 0), (1, 1), (1, 0), (1, -1), (1, -2), (1, -3), (0, -3), (0, -4), (1, -4), (2, -4), (1, -4)]),
                         ("next_lane0", 64, [(0, 0), (0, -1), (1, -1), (1, 0), (1, 1), (1, 2), (1, 3), (2, 3), (3, 3), (3, 4), (3, 3), (3, 2), (3, 1), (2, 1), (2, 0), (3, 0), (3, 1), (3, 2),
                                             (3, 3), (3, 2), (4, 2), (4, 1), (5, 1), (4, 1)]),
                         ("deep", 158, [(1, -1), (0, -1), (0, 0), (1, 0), (2, 0), (1, 0), (2, 0), (2, 1), (2, 2), (1, 2), (1, 1), (1, 0), (1, -1), (0, -1), (0, 0), (-1, 0), (0, 0), (0, -1)])):
        VIOLATOR_WALKS["inner_" + tag] = _osc(a) + tail
    # outer: to and fro, one step out at index a and back at once -- the point found there is one of the three that carry the final circle
    for tag, a in (("lane63", 65), ("next_lane0", 66), ("deep", 2 + 64 * 2 + 17)):
        x = (a - 1) % 2
        VIOLATOR_WALKS["outer_" + tag] = _osc(a) + [(x, 1), (x, 0), (1 - x, 0), (x, 0)]


_fill_violator_walks()
TINY = _tiny_pieces()
# finds every named walk must show (level, chunks advanced, lane); None = any lane
TINY_REACH = {"outer_lane63": ("outer", 0, 63), "outer_next_lane0": ("outer", 1, 0), "outer_deep": ("outer", 2, None),
              "middle_lane63": ("middle", 0, 63), "middle_next_lane0": ("middle", 1, 0), "middle_deep": ("middle", 2, None),
              "inner_lane63": ("inner", 0, 63), "inner_next_lane0": ("inner", 1, 0), "inner_deep": ("inner", 2, None)}


def tiny_case(name, **prm):
    return case(name, 80, 60, [([TINY[name]], [])], **dict(B_PRM, **prm))


def tiny_pinned(O, name):
    """[(case, fate)]: min_keep at 2 r (kept) and one ulp above (dropped), nothing a tap -- together they hold the device's radius to the oracle's, bit for bit"""
    piece, = O.cut_poly(TINY[name], np.zeros((60, 80), np.uint8))
    d = diameter(O, piece)
    return [(tiny_case(name, tap_diam=0.0, min_keep=d), "keep"), (tiny_case(name, tap_diam=0.0, min_keep=float(np.nextafter(d, np.inf))), "drop")]


# thresholds: axis-aligned pieces (integer perimeter) and one that is not
THRESH = {"bar_7": P([[10, 10], [17, 10]]), "ell_5_3": P([[10, 10], [15, 10], [15, 13]]), "square_6": P([[10, 10], [16, 10], [16, 16], [10, 16], [10, 10]]),
          "oblique": P([[10, 10], [17, 13], [12, 18]])}


def thresh_case(name, **prm):
    return case("thresh_" + name, 60, 40, [([THRESH[name]], [])], **prm)


def thresholds(O, name):
    """(prm overrides, branch, fate) at each threshold of one piece and one step to either side of it"""
    piece, = O.cut_poly(THRESH[name], np.zeros((40, 60), np.uint8))
    d = diameter(O, piece); n = len(piece); per = O.arc_length(piece, False)
    v = piece.reshape(-1, 2); ext = float(max(np.ptp(v[:, 0]), np.ptp(v[:, 1])))
    up, dn = float(np.nextafter(d, np.inf)), float(np.nextafter(d, 0.0))
    wide = dict(tap_max_per=1000.0, tap_max_v=1000); few = dict(tap_diam=50.0, tap_max_per=1000.0)
    out = [(dict(wide, tap_diam=d, min_keep=0.0), "circle", "tap"), (dict(wide, tap_diam=up, min_keep=0.0), "circle", "tap"), (dict(wide, tap_diam=dn, min_keep=0.0), "circle", "keep"),
           (dict(wide, tap_diam=dn, min_keep=100.0), "circle", "drop"),
           (dict(wide, tap_diam=0.0, min_keep=d), "circle", "keep"), (dict(wide, tap_diam=0.0, min_keep=dn), "circle", "keep"), (dict(wide, tap_diam=0.0, min_keep=up), "circle", "drop"),
           (dict(few, min_keep=0.0, tap_max_v=n), "circle", "tap"), (dict(few, min_keep=0.0, tap_max_v=n - 1), "many", "keep"),          # not tiny by its bbox
           (dict(few, min_keep=ext - 1.0, tap_max_v=n - 1), "circle", "keep"), (dict(few, min_keep=60.0, tap_max_v=n - 1), "circle", "drop")]
    if per == int(per):
        out += [(dict(tap_diam=50.0, min_keep=0.0, tap_max_v=1000, tap_max_per=per), "circle", "tap"), (dict(tap_diam=50.0, min_keep=0.0, tap_max_v=1000, tap_max_per=per - 0.5), "circle", "keep"),
                (dict(tap_diam=50.0, min_keep=60.0, tap_max_v=1000, tap_max_per=per - 0.5), "circle", "drop")]
    return out


# bbox shortcuts at their boundaries: (name, piece, prm, branch, fate)
def _scribble(ext, n, seed):
    """a unit walk of n points inside a box of exactly ext x ext"""
    rng = np.random.default_rng(seed)
    pts = [(10, 10)] + manhattan((10, 10), (10 + ext, 10)) + manhattan((10 + ext, 10), (10 + ext, 10 + ext))
    while len(pts) < n:
        x, y = pts[-1]; dx, dy = [(1, 0), (-1, 0), (0, 1), (0, -1)][int(rng.integers(0, 4))]
        if 10 <= x + dx <= 10 + ext and 10 <= y + dy <= 10 + ext:
            pts.append((x + dx, y + dy))
    return walk(pts)


BOX = [
    ("ext_equals_big", P([[10, 10], [18, 10]]), dict(tap_diam=6.0, min_keep=4.0), "circle", "keep"),
    ("ext_above_big", P([[10, 10], [19, 10]]), dict(tap_diam=6.0, min_keep=4.0), "big", "keep"),
    ("ext_equals_big_min_keep_larger", P([[10, 10], [10, 19]]), dict(tap_diam=3.0, min_keep=7.0), "circle", "keep"),
    ("many_ext_equals_min_keep_2", _scribble(8, 60, 1), dict(tap_diam=30.0, min_keep=6.0, tap_max_v=50), "many", "keep"),
    ("many_ext_below_min_keep_2", _scribble(7, 60, 2), dict(tap_diam=30.0, min_keep=6.0, tap_max_v=50), "circle", "keep"),
    ("many_ext_below_min_keep_2_dropped", _scribble(7, 60, 3), dict(tap_diam=30.0, min_keep=12.0, tap_max_v=50), "circle", "drop"),
    ("few_ext_equals_min_keep_2_tap", _scribble(8, 50, 4), dict(tap_diam=30.0, min_keep=6.0, tap_max_v=50), "circle", "tap"),
    ("vertices_one_too_many", _scribble(8, 51, 5), dict(tap_diam=30.0, min_keep=6.0, tap_max_v=50), "many", "keep"),
]


def box_case(i):
    name, piece, prm, _, _ = BOX[i]
    return case("box_" + name, 60, 40, [([piece], [])], **prm)


# two-point polylines of odd length: the tap centre lies on .5 and is rounded half to even.  (name, polyline, tap)
ODD = [("x_1_even", [[10, 10], [11, 10]], (10, 10)), ("x_1_odd", [[11, 14], [12, 14]], (12, 14)), ("x_3", [[20, 10], [23, 10]], (22, 10)), ("x_5", [[31, 10], [36, 10]], (34, 10)),
       ("y_1_even", [[10, 20], [10, 21]], (10, 20)), ("y_1_odd", [[14, 21], [14, 22]], (14, 22)), ("y_3", [[20, 20], [20, 23]], (20, 22)), ("y_5", [[30, 21], [30, 26]], (30, 24)),
       ("xy_1", [[10, 30], [11, 31]], (10, 30)), ("xy_1_odd", [[15, 31], [16, 32]], (16, 32)), ("xy_3", [[20, 30], [23, 33]], (22, 32)), ("xy_5", [[31, 31], [36, 36]], (34, 34)),
       ("x_3_y_5", [[42, 10], [45, 15]], (44, 12)), ("reversed_x_3", [[45, 25], [42, 25]], (44, 25))]
ODD_CASE = case("odd_two_point_taps", 60, 45, [([P(p) for _, p, _ in ODD], [])], tap_diam=20.0, min_keep=0.0)


# ---------------------------------------------------------------- C. paint
RADII = [0, 1, 30, 61, 62]
CANVASES = [(37, 29), (64, 32), (65, 33), (131, 70), (130, 70), (36, 29)]          # W mod 4 = 1, 0, 1, 3, 2, 0; smaller than one 64 x 32 tile, exactly one, one more


def probes(W, H, rows):
    return [P([[x, y] for x in range(W)]) for y in range(H)] if rows else [P([[x, y] for y in range(H)]) for x in range(W)]


def _uniq(a):
    out = []
    for v in a:
        if v not in out:
            out.append(v)
    return out


def paint_groups(W, H, r):
    """painting polylines by what they reach: name -> list of polylines (two vertices each, along the edge they stand at)"""
    offs = _uniq([r, r + 1, 63, 64, 65])          # just touching, just not; the last column of the seed pad, and beyond it
    ys = [3 + (H - 7) * k // max(1, len(offs) - 1) for k in range(len(offs))]; xs = [3 + (W - 7) * k // max(1, len(offs) - 1) for k in range(len(offs))]
    g = {}
    g["touch_left_right"] = [P([[-o, y], [-o, y + 1]]) for o, y in zip(offs, ys)] + [P([[W - 1 + o, y], [W - 1 + o, y - 1]]) for o, y in zip(offs, ys[::-1])]
    g["touch_top_bottom"] = [P([[x, -o], [x + 1, -o]]) for o, x in zip(offs, xs)] + [P([[x, H - 1 + o], [x - 1, H - 1 + o]]) for o, x in zip(offs, xs[::-1])]
    g["just_outside"] = [P([[-1, H // 2], [-1, H // 2 + 1]]), P([[W, H // 3], [W, H // 3 + 1]]), P([[W // 3, -1], [W // 3 + 1, -1]]), P([[W // 2, H], [W // 2 + 1, H]])]
    g["corners_near"] = [P([[0, 0], [1, 0]]), P([[W - 1, H - 1], [W - 2, H - 1]])]
    g["corners_far"] = [P([[W - 1, 0], [W - 1, 1]]), P([[0, H - 1], [0, H - 2]])]
    # a chain with a repeated position (the cut's (x, y), (x, y), (x + 1, y + 1)), steps of sqrt(2), and the next polyline far from the end of this one
    g["chains"] = [P([[4, 4], [5, 5], [6, 4], [7, 5]]), P([[W - 3, H - 4], [W - 5, H - 2]]), P([[W - 4, 2], [W - 4, 3]])]
    return g


def paint_case(W, H, r, group, rows):
    return case("paint_%dx%d_r%d_%s_%s" % (W, H, r, group, "rows" if rows else "columns"), W, H, [(paint_groups(W, H, r)[group], []), (probes(W, H, rows), [])], D_lines=float(2 * r + 1))


PAINT_GROUPS = ["touch_left_right", "touch_top_bottom", "just_outside", "corners_near", "corners_far", "chains"]


def crowded_case(rows):
    """so many vertices on a canvas so small that the stage takes the separable form by itself: vertices x (2 r + 1) > 4 W H"""
    W, H, r = 37, 29, 30
    return case("paint_crowded_%s" % ("rows" if rows else "columns"), W, H, [([snake(90, -35, -20, row=30), snake(60, 40, 40, row=20)], []), (probes(W, H, rows), [])], D_lines=float(2 * r + 1))


def takes_separable(O, c):
    """the stage's own switch, from the oracle's kept lines of the painting layer"""
    (lines, _), = raster_after(O, c, 1)[0]
    p = prm_of(c)
    return sum(len(l) for l in lines) * (2 * rad_lines(p) + 1) > 4 * c["W"] * c["H"]


def isolated_free(forb):
    """free pixels with no free neighbour in their row and none in their column"""
    f = np.pad(forb == 0, 1)
    return f[1:-1, 1:-1] & ~f[1:-1, :-2] & ~f[1:-1, 2:] & ~f[:-2, 1:-1] & ~f[2:, 1:-1]


# ---------------------------------------------------------------- D. tap filter
D_PRM = dict(D_taps=10.0, tap_diam=6.0, min_keep=0.0)          # tap radius 5: (3, 4) and (5, 0) lie exactly on the circle; pieces up to 6 px become taps


def _tap_cases():
    out = {}
    # (name, layers, accepted taps of the last layer)
    out["exactly_r"] = (case("exactly_r", 60, 50, [([], [(20, 20), (23, 24), (25, 20), (21, 25), (20, 15), (16, 17), (15, 20), (26, 21)])], **D_PRM), [(20, 20), (21, 25), (26, 21)])
    out["duplicates"] = (case("duplicates", 60, 50, [([], [(40, 40), (40, 40), (10, 10), (40, 40), (10, 10)])], **D_PRM), [(40, 40), (10, 10)])
    # off the canvas a candidate is never tested, not even against its own copy; its disc still counts for the candidates inside
    out["outside_canvas"] = (case("outside_canvas", 60, 50, [([], [(-2, 10), (-2, 10), (1, 14), (2, 14), (60, 30), (57, 34), (54, 30), (30, -5), (30, 0), (30, 1), (33, 53), (30, 49), (29, 50)])], **D_PRM),
                             [(-2, 10), (-2, 10), (2, 14), (60, 30), (54, 30), (30, -5), (30, 1), (33, 53), (29, 50)])
    # the layer's own line (radius-0 brush: exactly its vertices) forbids a candidate on it, not the one beside it
    out["on_own_line"] = (case("on_own_line", 60, 50, [([P([[10, 30], [30, 30]])], [(15, 30), (15, 31), (30, 30), (31, 30), (9, 30)])], **D_PRM), [(15, 31), (31, 30), (9, 30)])
    # given taps are filtered before the taps that come from lines: (12, 10) would lose against the line's (10, 10) the other way round
    out["given_before_line_taps"] = (case("given_before_line_taps", 60, 50, [([P([[9, 10], [11, 10]]), P([[39, 40], [41, 40]]), P([[20, 30], [22, 30]])], [(12, 10), (40, 45), (50, 5)])], **D_PRM),
                                     [(12, 10), (40, 45), (50, 5), (21, 30)])
    return out


TAPS = _tap_cases()
ACCEPTED = [63, 64, 65, 128, 129]


def accepted_case(n):
    """n taps 12 px apart, all accepted; then a candidate exactly r from the first of them, one exactly r from the LAST (the only accepted tap that hits it), and
    the same two at r^2 + 1, which are accepted"""
    g = [(6 + 12 * (k % 13), 6 + 12 * (k // 13)) for k in range(n)]
    f, l = g[0], g[-1]
    cand = g + [(f[0] + 3, f[1] + 4), (l[0] + 4, l[1] + 3), (l[0] - 5, l[1]), (f[0] + 1, f[1] + 5), (l[0] + 5, l[1] + 1)]
    return case("accepted_%d" % n, 170, 130, [([], cand)], **D_PRM), g + [(f[0] + 1, f[1] + 5), (l[0] + 5, l[1] + 1)]


def tap_stamp_case(rows):
    """the discs the accepted taps leave for the NEXT layer (the filter itself compares with its list, not with the raster): taps in two corners, on the circle's
    reach outside the canvas and one beyond it, read back by a probe layer"""
    W, H = 45, 38
    taps = [(0, 0), (W - 1, H - 1), (-5, 12), (-6, 24), (22, -5), (33, -6), (W + 4, 14), (W + 5, 26), (12, H + 4), (24, H + 5), (22, 19)]
    return case("taps_stamp_%s" % ("rows" if rows else "columns"), W, H, [([], taps), (probes(W, H, rows), [])], D_taps=10.0)


# ---------------------------------------------------------------- E. step_px
STEP_SAME = [0.25, 1.0, -3.0]          # max(1, step_px) = 1: the answer of step 1
STEP_ABOVE = [1.5, 2.5, 40.0]


def step_case():
    rng = np.random.default_rng(1010)
    mk = lambda n: [P(np.cumsum(rng.integers(-25, 26, (int(rng.integers(2, 7)), 2)), axis=0) + rng.integers(40, 120, 2)) for _ in range(n)]
    return case("step_px", 180, 150, [(mk(10), [(30, 30), (100, 90)]), (mk(12), [(32, 31), (150, 20)]), (mk(12), [])], tap_diam=12.0, min_keep=5.0, D_lines=9.0, D_taps=8.0)


# ---------------------------------------------------------------- the lists the test files run
def small_cases():
    """every case but the paint grid and the large layer: name -> case"""
    out = dict(CUT)
    for n in TINY:
        out["tiny_" + n] = tiny_case(n)
    for i, b in enumerate(BOX):
        out["box_" + b[0]] = box_case(i)
    out[ODD_CASE["name"]] = ODD_CASE
    for n, (c, _) in TAPS.items():
        out["taps_" + n] = c
    for n in ACCEPTED:
        out["taps_accepted_%d" % n] = accepted_case(n)[0]
    for rows in (True, False):
        c = tap_stamp_case(rows); out[c["name"]] = c
    return out
