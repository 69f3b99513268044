"""The drawings of the --occlude tests (tests/test_occlude_host.py on the CPU, tests/test_gpu_occlude.py on the device): named cases, the hand-worked
answers of the rule as literals, and seeded random drawings, rectilinear and oblique.  A drawing is (strokes, levels, rings, ring_levels) in lists;
arrays() gives the six arrays of Device.gcode_occlude."""
import math
import random

import numpy as np

TOP = 1 << 30


def sq(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def closed(ring):
    return list(ring) + [ring[0]]


def offsets(lists):
    return np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)


def arrays(case):
    strokes, levels, rings, ring_levels = case
    pts = np.asarray([q for p in strokes for q in p], np.int64).reshape(-1, 2).astype(np.int32)
    rpts = np.asarray([q for p in rings for q in p], np.int64).reshape(-1, 2).astype(np.int32)
    return offsets(strokes), pts, np.asarray(levels, np.int32), offsets(rings), rpts, np.asarray(ring_levels, np.int32)


def reverse_stroke(case, k):
    strokes, levels, rings, ring_levels = case
    return [s[::-1] if i == k else s for i, s in enumerate(strokes)], levels, rings, ring_levels


# (drawing, output strokes, origin or None, the counts that are stated): the hand-worked answers of the rule
TRIANGLE = [(0, 0), (9, 0), (0, 7)]
HAND = [
    (([[(0, 5), (20, 5)]], [0], [sq(5, 0, 15, 10)], [1]), [[(0, 5), (5, 5)], [(15, 5), (20, 5)]], None, dict(cut=1, pieces=2)),
    (([closed(sq(0, 0, 10, 10)), closed(sq(5, 5, 15, 15))], [0, 1], [sq(0, 0, 10, 10), sq(5, 5, 15, 15)], [0, 1]),
     [[(0, 0), (10, 0), (10, 5)], [(5, 10), (0, 10), (0, 0)], closed(sq(5, 5, 15, 15))], [0, 0, 1], dict(segments=8, whole=6, cut=2)),
    (([closed(sq(0, 0, 10, 10)), closed(sq(10, 0, 20, 10))], [0, 1], [sq(0, 0, 10, 10), sq(10, 0, 20, 10)], [0, 1]),
     [closed(sq(0, 0, 10, 10)), closed(sq(10, 0, 20, 10))], [0, 1], dict(whole=8)),
    (([[(0, 10), (30, 10)]], [0], [sq(5, 0, 25, 20), sq(10, 5, 20, 15)], [3, 3]), [[(0, 10), (5, 10)], [(10, 10), (20, 10)], [(25, 10), (30, 10)]], None, {}),
    (([[(0, 0), (10, 7)]], [0], [[(3, -5), (30, -5), (30, 30), (3, 30)]], [1]), [[(0, 0), (3, 2)]], None, {}),
]
# the triangle case is stated with a stroke that leaves the sheet: the uploaded form takes it shifted onto the sheet by (TRI_SHIFT, 0), rings and all
TRI_SHIFT = 5
HAND_TRIANGLE = (([[(-5, 3), (20, 3)]], [0], [TRIANGLE], [1]), [[(-5, 3), (0, 3)], [(5, 3), (20, 3)]])


def shifted(case, dx, dy=0):
    strokes, levels, rings, ring_levels = case
    mv = lambda ls: [[(x + dx, y + dy) for x, y in p] for p in ls]
    return mv(strokes), levels, mv(rings), ring_levels


def comb(teeth=70, x0=10):
    """one ring: a bar with `teeth` teeth, each 2 wide and 4 apart, standing on it; a stroke across all teeth leaves teeth + 1 pieces"""
    ring = [(x0, 0), (x0 + 4 * teeth, 0)]
    for k in reversed(range(teeth)):
        x = x0 + 4 * k
        ring += [(x + 4, 5), (x + 3, 5), (x + 3, 20), (x + 1, 20), (x + 1, 5)]
    ring += [(x0, 5)]
    return [[(0, 10), (x0 + 4 * teeth + 10, 11)]], [0], [ring], [1]


def polygon(edges=200, r=1000, c=2000):
    ring = [(c + round(r * math.cos(2 * math.pi * k / edges)), c + round(r * math.sin(2 * math.pi * k / edges))) for k in range(edges)]
    strokes = [[(500, 500), (3500, 3400)], [(900, 2000), (3100, 2000), (3100, 2100), (900, 2050)], [(2000, 900), (2000, 3100)], [(1000, 1000), (1300, 1290), (2000, 2000)],
               [(c + r, c), (c + r + 50, c + 40)]]
    return strokes, [0] * len(strokes), [ring], [7]


def scatter(seed=5, strokes=300, shapes=40, side=4000):
    rnd = random.Random(seed)
    rings, ring_levels = [], []
    for lv in sorted(rnd.sample(range(1, 200), shapes)):
        x, y, w, h = rnd.randrange(side - 400), rnd.randrange(side - 400), rnd.randrange(40, 400), rnd.randrange(40, 400)
        kind = rnd.randrange(3)
        if kind == 0:
            rings.append(sq(x, y, x + w, y + h))
        elif kind == 1:
            rings.append([(x, y), (x + w, y + h // 3), (x + w // 2, y + h)])
        else:
            rings += [sq(x, y, x + w, y + h), sq(x + w // 4, y + h // 4, x + w // 2, y + h // 2)]; ring_levels.append(lv)
        ring_levels.append(lv)
    out, levels = [], []
    for _ in range(strokes):
        x, y = rnd.randrange(side - 300), rnd.randrange(side - 300)
        p = [(x, y)]
        for _ in range(rnd.randrange(1, 4)):
            q = (p[-1][0] + rnd.randrange(-150, 300), p[-1][1] + rnd.randrange(-150, 300))
            q = (min(max(q[0], 0), side), min(max(q[1], 0), side))
            if q != p[-1]:
                p.append(q)
        if len(p) >= 2:
            out.append(p); levels.append(rnd.randrange(0, 200))
    return out, levels, rings, ring_levels


def sliver(k=(1 << 29) + 1):
    """coordinates at 0 and 2^30: the long stroke meets the ring at k / 2^30 and at (k + about k / 2^60) / 2^30, two parameters that are one double"""
    return [[(0, 0), (TOP, 1)]], [0], [[(k, 0), (k + 1, TOP), (k, TOP)]], [1]


def cases():
    c = {f"hand_{i}": h[0] for i, h in enumerate(HAND)}
    c["hand_triangle"] = shifted(HAND_TRIANGLE[0], TRI_SHIFT)
    c["hand_triangle_reversed"] = reverse_stroke(c["hand_triangle"], 0)
    ell = [(5, 0), (25, 0), (25, 10), (15, 10), (15, 20), (5, 20)]
    c["along_an_edge_partly"] = ([[(0, 0), (20, 0)], [(20, 10), (0, 10)], [(0, 10), (30, 10)]], [0, 0, 0], [sq(5, 0, 15, 10), ell], [1, 2])
    c["along_an_edge_wholly"] = ([[(5, 0), (15, 0)], [(15, 10), (25, 10)], [(25, 10), (15, 10), (5, 10)]], [0, 0, 0], [ell], [1])
    c["through_convex_vertices"] = ([[(0, 10), (30, 10)], [(10, 30), (10, 0)], [(0, 20), (20, 0)]], [0, 0, 0], [[(10, 0), (20, 10), (10, 20), (0, 10)]], [1])
    c["through_a_reflex_vertex"] = ([[(0, 10), (30, 10)], [(30, 10), (0, 10)], [(15, 0), (15, 30)]], [0, 0, 0], [[(5, 0), (25, 0), (25, 20), (15, 10), (5, 20)]], [1])
    c["touching_an_apex"] = ([[(0, 10), (20, 10)], [(10, 10), (10, 30)]], [0, 0], [[(5, 0), (15, 0), (10, 10)]], [1])
    c["two_shapes_touch_on_the_stroke"] = ([[(0, 10), (30, 10)], [(30, 10), (0, 10)]], [0, 0], [[(5, 10), (10, 5), (15, 10), (10, 15)], [(15, 10), (20, 5), (25, 10), (20, 15)]], [1, 2])
    c["degenerate_rings"] = ([[(0, 5), (20, 5)], [(0, 0), (20, 20)]], [0, 1],
                             [[(7, 5)], [(3, 5), (9, 5)], [(5, 0), (5, 0), (15, 0), (15, 10), (15, 10), (5, 10)], [(2, 2), (2, 2)], [(0, 0), (20, 20)]], [1, 1, 2, 2, 3])
    c["levels_decide"] = ([[(0, 5), (20, 5)], [(0, 6), (20, 6)], [(0, 7), (20, 7)]], [0, 1, 2], [sq(5, 0, 15, 10), sq(2, 4, 8, 8)], [1, 2])
    c["nothing_above"] = ([[(0, 5), (20, 5), (20, 9)], [(3, 3), (9, 9)]], [4, 5], [sq(5, 0, 15, 10), sq(2, 2, 30, 30)], [1, 4])
    c["no_rings"] = ([[(0, 5), (20, 5), (20, 9)], [(3, 3), (9, 9)]], [0, 0], [], [])
    c["all_hidden"] = ([[(6, 5), (9, 5), (9, 8)], [(7, 7), (8, 8)]], [0, 0], [sq(5, 0, 15, 10)], [1])
    # the two shapes leave (49.2, 49.4) of the strokes visible: both ends round to (49, 0), the piece is dropped, and nothing else is left
    c["collapsing_piece"] = ([[(0, 0), (100, 0)], [(100, 0), (0, 0)]], [0, 0], [[(0, -5), (49, -5), (50, 20), (0, 20)], [(49, -10), (100, -10), (100, 15), (50, 15)]], [1, 2])
    c["cut_at_a_vertex_of_the_stroke"] = ([[(0, 5), (5, 5), (10, 5), (15, 5), (20, 5)], [(0, 0), (5, 0), (5, 10), (0, 10)]], [0, 0], [sq(5, 0, 15, 10)], [1])
    c["comb_of_70_teeth"] = comb()
    c["polygon_of_200_edges"] = polygon()
    c["scatter"] = scatter()
    c["sliver_at_2_to_30"] = sliver()
    return c


def random_rectilinear(seed):
    rnd = random.Random(1000 + seed)
    rings, ring_levels = [], []
    for lv in sorted(rnd.randrange(0, 4) for _ in range(rnd.randrange(0, 5))):
        x, y = rnd.randrange(-2, 10), rnd.randrange(-2, 10)
        rings.append(sq(x, y, x + rnd.randrange(1, 8), y + rnd.randrange(1, 8))); ring_levels.append(lv)
    strokes, levels = [], []
    for _ in range(rnd.randrange(1, 7)):
        p = [(rnd.randrange(0, 13), rnd.randrange(0, 13))]
        for _ in range(rnd.randrange(1, 5)):
            x, y = p[-1]
            q = (rnd.randrange(0, 13), y) if rnd.random() < 0.5 else (x, rnd.randrange(0, 13))
            if q != p[-1]:
                p.append(q)
        if len(p) >= 2:
            strokes.append(p); levels.append(rnd.randrange(0, 4))
    return strokes, levels, rings, ring_levels


def random_oblique(seed):
    """at most 8 strokes and 3 shapes on a grid so small that vertices on lines, collinear edges and shared points are the rule"""
    rnd = random.Random(seed)
    rings, ring_levels = [], []
    for lv in sorted(rnd.sample(range(0, 5), rnd.randrange(0, 4))):
        for _ in range(rnd.randrange(1, 3)):
            rings.append([(rnd.randrange(-2, 14), rnd.randrange(-2, 14)) for _ in range(rnd.randrange(1, 6))]); ring_levels.append(lv)
    strokes, levels = [], []
    for _ in range(rnd.randrange(1, 9)):
        p = [(rnd.randrange(0, 13), rnd.randrange(0, 13))]
        for _ in range(rnd.randrange(1, 4)):
            q = (rnd.randrange(0, 13), rnd.randrange(0, 13))
            if q != p[-1]:
                p.append(q)
        if len(p) >= 2:
            strokes.append(p); levels.append(rnd.randrange(0, 5))
    return strokes, levels, rings, ring_levels


# ------------------------------------------------------------------ the whole tool
# nested groups, an unfilled line between two filled elements, a path with a hole, an open polyline and a rectangle that states no fill; every segment is
# axis-parallel, so the unit steps of a stroke are its own.  Elements that drew: rect 0, line 1, path 2 (two subpaths), polyline 3, rect 4.
TOOL_SVG = b"""<svg xmlns="http://www.w3.org/2000/svg" width="200" height="200" viewBox="0 0 200 200">
 <g stroke="#00f"><g><rect x="20" y="20" width="100" height="80" fill="#ccc"/><desc>nothing drawn</desc></g><line x1="10" y1="60" x2="190" y2="60"/></g>
 <g><path d="M60 50 H160 V150 H60 Z M80 70 H140 V130 H80 Z" fill="red" stroke="#f00"/></g>
 <polyline points="0,140 200,140" stroke="#00f" fill="none"/>
 <rect x="150" y="10" width="40" height="30" stroke="#00f"/>
</svg>
"""
TOOL_ELEMENTS = [0, 1, 2, 2, 3, 4]
TOOL_FILL_GROUPS = [0, -1, 2, 2, -1, -1]
TOOL_ARGS = ["--occlude", "--scale", "1", "--margin-mm", "0", "--steps-per-mm", "4"]
# a shape half off the sheet (the drawing is 330 mm wide, the page 210): the triangle's apex lies 120 mm beyond the edge.  Clamped to the sheet its sides would
# change their slope ON the sheet and the stroke at y = 80 would show again from x = 186 mm; under --clip the rings are not clamped and it stays hidden
TOOL_SVG_OFF_SHEET = b"""<svg xmlns="http://www.w3.org/2000/svg" width="330" height="200" viewBox="0 0 330 200">
 <path d="M0 80 H280" stroke="#00f" fill="none"/><path d="M0 120 H205 V60" stroke="#00f" fill="none"/>
 <path d="M150 50 L330 100 L150 150 Z" fill="#f00" stroke="#f00"/>
</svg>
"""


def unit_steps(strokes):
    """the unit steps of axis-parallel or diagonal strokes, as sorted point pairs, in order"""
    out = []
    for s in strokes:
        for (ax, ay), (bx, by) in zip(s[:-1], s[1:]):
            n = max(abs(bx - ax), abs(by - ay)); ux, uy = (bx - ax) // n, (by - ay) // n
            assert (ax + n * ux, ay + n * uy) == (bx, by)
            out += [tuple(sorted(((ax + i * ux, ay + i * uy), (ax + (i + 1) * ux, ay + (i + 1) * uy)))) for i in range(n)]
    return out


class OccludeDouble:
    """occlude_fn of orip.svg.build_stream_from_svg through the doubles: the rings converted by occlude_double.rings_to_steps, the pass by occlude_numpy"""
    def __init__(self): self.calls = 0; self.out = None; self.rings = None; self.level = None

    def __call__(self, paths, off, pts, level, ring_sub, ring_level, m, clamp):
        import occlude_double as OD
        r_off, r_pts = OD.rings_to_steps(np.asarray(paths[0]), np.asarray(paths[1]), np.asarray(ring_sub).tolist(), m, clamp)
        self.rings = (r_off, r_pts, clamp); self.level = np.asarray(level)
        self.out = OD.occlude_numpy(off, pts, level, r_off, r_pts, ring_level)
        self.calls += 1
        return self.out
