"""TEST INFRASTRUCTURE: the inputs of the --simplify-mm tests (tests/test_simplify_host.py on the double, tests/test_gpu_simplify.py on the device): the rule's
hand-worked answers, the smallest shapes that can break the kernel (wave edges, the local-finish threshold, products that need all 128 bits, mixtures) and
the drawing of the whole-tool tests as G-code and as SVG."""
import numpy as np

from orip.lib import SIMPLIFY_LOCAL as S          # the points one wave finishes alone: where the host states it

TOP = 1 << 30


def strokes(lists):
    """[[(x, y), ...], ...] -> (off, pts)"""
    off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
    return off, np.asarray([q for p in lists for q in p], np.int64).reshape(-1, 2).astype(np.int32)


def staircase():
    return [(k // 2 + k % 2, k // 2) for k in range(201)]


# points, tol4, kept: worked by hand from the rule in include/orip.h
HAND = [
    ([(0, 0), (5, 0), (10, 0)], 0, [0, 2]),
    ([(0, 0), (15, 0), (10, 0)], 0, [0, 1, 2]),                               # beyond the end of the chord: not on the segment
    ([(0, 0), (10, 1), (20, 0)], 4, [0, 2]),                                  # exactly one step away: 16 K == tol4^2 L is not kept
    ([(0, 0), (10, 1), (20, 0)], 3, [0, 1, 2]),
    ([(0, 0), (5, 2), (10, -2), (15, 2), (20, 0)], 8, [0, 4]),
    ([(0, 0), (5, 2), (10, -2), (15, 2), (20, 0)], 7, [0, 1, 2, 3, 4]),       # a three-way tie, the lowest index first
    ([(0, 0), (3, 1), (0, 0)], 400, [0, 1, 2]),                               # a loop is never collapsed
    ([(0, 0), (4, 0), (0, 0), (4, 0), (0, 0)], 0, [0, 1, 4]),                 # degenerate, then the same points again on the segment
]
STAIR_COUNTS = {3: 2, 2: 199, 0: 201}                                        # tol4 -> points kept of the staircase
# the hand-worked cases use negative coordinates; the device takes 0 .. 2^30, so there they are moved (the rule only sees differences)
SHIFT = 7


def bumpy(interior, peaks, peak=50):
    """a stroke with `interior` interior points on a low zigzag (1 or 2 steps over the chord), those whose INDEX is in `peaks` `peak` steps higher"""
    return [(10 * i + 5, 100 + (0 if i in (0, interior + 1) else 1 + i % 2 + (peak if i in peaks else 0))) for i in range(interior + 2)]


def arc(n, peak_at, peak=400):
    """n points along a shallow, uneven arc, the point of index peak_at `peak` steps off it"""
    return [(3 * i + 2, 1000 + (i * i) % 7 + (i * (n - 1 - i)) // (4 * n) + (peak if i == peak_at else 0)) for i in range(n)]


def egcd(a, b):
    """(g, s, t) with s a + t b == g"""
    if b == 0:
        return a, 1, 0
    g, s, t = egcd(b, a % b)
    return g, t, s - (a // b) * t


def lattice_point(dx, dy, c):
    """the lattice point P (relative to the chord's first end) with cross(P, d) == c and 0 <= P . d < L: extended Euclid gives (u, v) with u dy - v dx == 1"""
    g, s, t = egcd(dy, dx)
    assert g == 1
    u, v = s, -t
    assert u * dy - v * dx == 1
    L = dx * dx + dy * dy
    k = -((c * (u * dx + v * dy)) // L)
    P = (c * u + k * dx, c * v + k * dy)
    assert P[0] * dy - P[1] * dx == c and 0 <= P[0] * dx + P[1] * dy < L
    return P


def cross_pair():
    """a chord with coprime dx, dy next to 2^30 and two points whose cross products with it differ by exactly 1 at 2^59, one step apart: whichever is
    taken first, the other lies within two steps of the new segment and goes, so the kept one tells which product was found larger"""
    dx, dy = TOP - 1, TOP - 2
    g, s, t = egcd(dy, dx)
    u, v = s, -t
    assert g == 1 and u * dy - v * dx == 1 and max(abs(u), abs(v)) <= 2
    P = (3 << 28, 1 << 28)
    Q = (P[0] + u, P[1] + v)
    cP, cQ = P[0] * dy - P[1] * dx, Q[0] * dy - Q[1] * dx
    assert cQ - cP == 1 and cP >= 1 << 58 and 0 < P[0] * dx + P[1] * dy < dx * dx + dy * dy
    return (0, 0), (dx, dy), P, Q                                             # Q has the larger product


# (dx, dy, tol4, c): 16 c^2 and tol4^2 L differ by less than one part in 2^64, found by a search over tol4; the first is below the threshold, the second above
NEAR = {"below": (1073609458, 1073609995, 71650, 27196789420774), "above": (1073608762, 1073609667, 121012, 45933514471137)}


def near_threshold(which):
    dx, dy, tol4, c = NEAR[which]
    L = dx * dx + dy * dy
    diff = 16 * c * c - tol4 * tol4 * L
    assert diff != 0 and (diff > 0) == (which == "above") and abs(diff) << 64 < 16 * c * c
    A = (1 << 16, 1 << 16)
    P = lattice_point(dx, dy, c)
    pts = [A, (A[0] + P[0], A[1] + P[1]), (A[0] + dx, A[1] + dy)]
    assert all(0 <= v <= TOP for q in pts for v in q)
    return pts, tol4


def ring(n, r, cx, cy, phase=0.0):
    t = np.linspace(0.0, 2.0 * np.pi, n) + phase
    P = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1).round().astype(np.int64)
    P[-1] = P[0]
    return [tuple(q) for q in P.tolist()]


def figure_eight(n=120, r=500, cx=3000, cy=3000):
    """from the crossing round the right loop, through the crossing, round the left loop, back to the crossing"""
    t = np.linspace(0.0, 2.0 * np.pi, n)
    right = np.stack([cx + r - r * np.cos(t), cy + r * np.sin(t)], 1).round().astype(np.int64)
    left = np.stack([cx - r + r * np.cos(t), cy + r * np.sin(t)], 1).round().astype(np.int64)
    right[-1] = right[0]; left[0] = left[-1] = right[0]
    return [tuple(q) for q in right.tolist()] + [tuple(q) for q in left[1:].tolist()]


def walk(n=40000, seed=11):
    """a random walk, every step one of the eight neighbours: no two consecutive points equal"""
    rng = np.random.default_rng(seed)
    d = np.array([(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)], np.int64)[rng.integers(0, 8, n - 1)]
    P = np.concatenate([[[0, 0]], np.cumsum(d, 0)]) + 20000
    return [tuple(q) for q in P.tolist()]


def mixture(seed=2):
    """many two-point strokes between long ones (one of them longer than a wave finishes alone): the scan, and strokes without a task"""
    rng = np.random.default_rng(seed)
    two = lambda k: [[(int(a), int(b)), (int(a) + 1 + int(c), int(b) + int(e))] for a, b, c, e in rng.integers(0, 5000, (k, 4))]
    return two(50) + [arc(300, 150)] + two(70) + [arc(S + 500, 77)] + two(1) + [ring(200, 700, 2000, 2000)] + two(129)


def cases():
    """name -> (off, pts, tol4): every shape of the device test"""
    c = {}
    for k, (pts, tol4, _) in enumerate(HAND):
        c[f"hand_{k}"] = strokes([[(x + SHIFT, y + SHIFT) for x, y in pts]]) + (tol4,)
    for tol4 in STAIR_COUNTS:
        c[f"staircase_{tol4}"] = strokes([staircase()]) + (tol4,)
    for n in (62, 63, 64, 65, 127, 128, 129):                                 # interior points: the lanes' last round is full, one short, one over
        c[f"wave_{n}_first"] = strokes([bumpy(n, {1})]) + (4,)
        c[f"wave_{n}_last"] = strokes([bumpy(n, {n})]) + (4,)
        if n >= 64:
            c[f"wave_{n}_at_64"] = strokes([bumpy(n, {64})]) + (4,)
        c[f"wave_{n}_tie"] = strokes([bumpy(n, {1, n})]) + (4,)
    for n in (S - 1, S, S + 1, 2 * S + 3):                                    # the top-level point is the last interior one: one child is empty, the other goes on
        c[f"local_{n}"] = strokes([arc(n, n - 2)]) + (6,)
    A, B, P, Q = cross_pair()
    c["cross_larger_second"] = strokes([[A, P, Q, B]]) + (8,)
    c["cross_larger_first"] = strokes([[A, Q, P, B]]) + (8,)
    for which in NEAR:
        pts, tol4 = near_threshold(which)
        c[f"near_{which}"] = strokes([pts]) + (tol4,)
    c["mixture"] = strokes(mixture()) + (4,)
    c["two_points_only"] = strokes([[(1, 1), (5, 9)], [(5, 9), (1, 1)], [(0, 0), (TOP, TOP)]]) + (40,)
    c["ring"] = strokes([ring(200, 900, 1000, 1000, 0.3)]) + (8,)
    c["figure_eight"] = strokes([figure_eight()]) + (12,)
    c["corners"] = strokes([[(0, 0), (TOP, 0), (TOP, TOP), (0, TOP), (0, 0)], [(0, TOP), (TOP // 2, TOP // 2 + 1), (TOP, 0)]]) + (TOL4_MAX,)
    c["walk"] = strokes([walk()]) + (2,)
    return c


TOL4_MAX = (1 << 17) - 1


# ------------------------------------------------------------------ the drawing of the whole-tool tests
def _subdivide(corners, rng):
    """a polyline through the corners (in steps; every leg axis-aligned or at 45 degrees), every leg cut into pieces of 1 .. 40 steps"""
    out = [corners[0]]
    for a, b in zip(corners[:-1], corners[1:]):
        n = max(abs(b[0] - a[0]), abs(b[1] - a[1]))
        assert abs(b[0] - a[0]) in (0, n) and abs(b[1] - a[1]) in (0, n)
        ux, uy = (b[0] - a[0]) // n, (b[1] - a[1]) // n
        k = 0
        while k < n:
            k = min(n, k + int(rng.integers(1, 41)))
            out.append((a[0] + ux * k, a[1] + uy * k))
    return out


COPIES = 6


def _lines(seed=4):
    """COPIES times, each 60 steps further along both axes: a closed outline, a zigzag, a subdivided line and a plain one"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(COPIES):
        mv = lambda c: [(x + 60 * k, y + 60 * k) for x, y in c]
        out += [_subdivide(mv([(400, 400), (2400, 400), (3400, 1400), (3400, 3000), (2000, 4400), (400, 4400), (400, 400)]), rng),
                _subdivide(mv([(4000, 500), (4600, 1100), (5200, 500), (5800, 1100), (6400, 500), (6400, 2500), (4000, 2500)]), rng),
                _subdivide(mv([(4000, 3000), (6000, 3000)]), rng), mv([(4000, 3200), (6000, 3200)])]
    return out


def _curves():
    t = np.linspace(0.0, 2.0 * np.pi, 241)
    circle = np.stack([150.0 + 15.0 * np.cos(t), 200.0 + 15.0 * np.sin(t)], 1)
    s = np.arange(300)
    sine = np.stack([20.0 + 0.25 * s, 250.0 + 12.0 * np.sin(s / 20.0)], 1)
    spiral = np.stack([60.0 + (2.0 + 0.04 * s) * np.cos(s / 9.0), 180.0 + (2.0 + 0.04 * s) * np.sin(s / 9.0)], 1)
    return [c.round(3).tolist() for c in (circle, sine, spiral)]


def tool_strokes_mm(curves=True):
    """the strokes in mm at 40 steps per mm: the subdivided lines (multiples of a step), then a circle, a sine and a spiral flattened finely"""
    out = [[(x / 40.0, y / 40.0) for x, y in p] for p in _lines()]
    return out + [[tuple(q) for q in c] for c in _curves()] if curves else out


def tool_gcode(curves=True):
    out = ["G21", "G90", "M5"]
    for s in tool_strokes_mm(curves):
        out += ["G0 X%.3f Y%.3f" % tuple(s[0]), "M3"] + ["G1 X%.3f Y%.3f" % tuple(q) for q in s[1:]] + ["M5"]
    return "\n".join(out) + "\n"


def tool_svg():
    """the same strokes as <polyline> elements, the lines red and the curves blue"""
    n_lines = len(_lines())
    body = "".join('<polyline fill="none" stroke="%s" points="%s"/>' % ("#f00" if i < n_lines else "#00f", " ".join("%.3f,%.3f" % tuple(q) for q in s))
                   for i, s in enumerate(tool_strokes_mm()))
    return ('<svg xmlns="http://www.w3.org/2000/svg" width="210" height="297" viewBox="0 0 210 297">' + body + "</svg>").encode()


LINE_STROKES, LINE_CORNERS, CURVES = 4 * COPIES, (7 + 7 + 2 + 2) * COPIES, 3
TOOL_MM = 0.1                                                                 # tol4 == 16 at 40 steps per mm
TOOL_SVG_ARGS = ["--simplify-mm", "0.1", "--pen-colors", "#f00,#00f"]
