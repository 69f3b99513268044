"""Named drawings for --dedup, each small: cases() -> {name: (off int64, pts int32 [total, 2], group int32 [n] or None, n_groups)}; random drawings of the kind
the rule was tried on; and the two tool inputs.  The answers come from tests/dedup_double.py; HAND holds the few that are written down by hand."""
import numpy as np

TOP = 1 << 30
L = 7                                               # the side of the grid's squares


def strokes(lists):
    off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
    return off, np.asarray([q for p in lists for q in p], np.int32).reshape(-1, 2)


def square(x, y, s=L):
    return [(x, y), (x + s, y), (x + s, y + s), (x, y + s), (x, y)]


def grid_of_squares(k=3, s=L, x0=10, y0=10):
    return [square(x0 + i * s, y0 + j * s, s) for j in range(k) for i in range(k)]


def along(p0, d, ts):
    return [(p0[0] + t * d[0], p0[1] + t * d[1]) for t in ts]


def direction_case(p0, d):
    """on one line of direction d: a stroke, a longer one over it drawn backwards, a stroke that only touches, and a parallel neighbour"""
    return [along(p0, d, [2, 5]), along(p0, d, [7, 0]), along(p0, d, [7, 9]), along((p0[0] + 1, p0[1]), d, [2, 5])]


def staggered(n, seed):
    """n segments [3 i, 3 i + 5] on one line in a shuffled drawing order, one of them left out, then one stroke over all of them"""
    rng = np.random.default_rng(seed)
    idx = [i for i in rng.permutation(n + 1).tolist() if i != n // 2]
    return [[(100 + 3 * i, 50), (100 + 3 * i + 5, 50)] for i in idx] + [[(90, 50), (100 + 3 * n + 20, 50)]]


def cases():
    c = {}

    def add(name, lists, group=None, n_groups=1):
        off, pts = strokes(lists)
        c[name] = (off, pts, None if group is None else np.asarray(group, np.int32), n_groups)
    add("out_and_back", [[(3, 3), (9, 6), (3, 3)]])
    add("two_squares", [square(5, 5), square(5 + L, 5)])
    add("grid_3x3", grid_of_squares())
    add("short_inside_a_later_long", [[(10, 4), (20, 4)], [(0, 9), (0, 4), (30, 4), (30, 9)]])
    add("long_first_then_shorts", [[(0, 4), (40, 4)], [(5, 4), (9, 4), (12, 4)], [(50, 4), (30, 4)], [(40, 4), (20, 4), (20, 8)]])
    add("beyond_the_start", [[(10, 2), (20, 2), (0, 2)]])
    add("touching_only", [[(0, 0), (5, 0)], [(5, 0), (9, 0)], [(9, 0), (9, 4), (5, 0)], [(2, 3), (2, 0)], [(0, 5), (5, 0)], [(3, 2), (6, 5)]])
    add("two_groups", [[(0, 0), (8, 0), (8, 8)], [(8, 0), (0, 0)], [(8, 8), (8, 0), (0, 0)], [(0, 0), (8, 0)]], [0, 1, 1, 0], 2)
    for name, p0, d in (("horizontal", (4, 9), (1, 0)), ("vertical", (9, 4), (0, 1)), ("diagonal_up", (3, 3), (1, 1)), ("diagonal_down", (3, 40), (1, -1)),
                        ("direction_7_-3", (5, 60), (7, -3)), ("direction_-3_7", (60, 5), (-3, 7))):
        add(name, direction_case(p0, d))
    # lines equal in all but one key word: each pair overlaps in tau and must not touch each other's ink
    add("differ_in_the_sign_of_uy", [[(0, 4), (4, 8)], [(0, 4), (4, 0)], [(1, 5), (3, 7)], [(3, 1), (1, 3)]])
    add("differ_in_the_low_bits_of_c", [[(0, 0), (10, 0)], [(0, 1), (10, 1)], [(2, 1), (8, 1)], [(2, 0), (12, 0)]])
    y0, w = TOP - 100, 1 << 29
    add("differ_in_the_high_bits_of_c", [[(0, y0), (w, y0 + 1)], [(0, y0 + 8), (w, y0 + 9)], [(w, y0 + 1), (0, y0)], [(2 * w, y0 + 10), (0, y0 + 8)]])       # c apart by exactly 2^32
    add("c_near_the_top", [[(1, TOP), (TOP, 0)], [(TOP, 0), (1, TOP)], [(0, TOP), (TOP - 1, 0)], [(0, 0), (TOP, TOP)], [(TOP, TOP), (5, 5), (0, 0)]])
    add("differ_in_the_group", [[(0, 0), (10, 0)], [(2, 0), (8, 0)], [(2, 0), (8, 0)]], [0, 1, 0], 64)
    for n in (63, 64, 65, 129):
        add(f"staggered_{n}", staggered(n, n))
    add("dashes_200_then_one", [[(10 * i + 5, 7), (10 * i + 9, 7)] for i in range(200)] + [[(0, 7), (2010, 7)]])
    add("dashes_200_then_one_backwards", [[(7, 10 * i + 5), (7, 10 * i + 9)] for i in range(200)] + [[(3, 2010), (7, 2010), (7, 0), (3, 0)]])
    # more than 64 x 64 positions on one line: the backward search steps over whole blocks of 64 positions and of 64 blocks
    add("dashes_5000_then_one", [[(10 * i + 5, 9), (10 * i + 9, 9)] for i in range(5000)] + [[(0, 9), (50010, 9)]])
    add("one_then_dashes_5000", [[(0, 9), (50010, 9)]] + [[(10 * i + 5, 9), (10 * i + 9, 9)] for i in range(5000)] + [[(50000, 9), (50020, 9)]])
    add("walls_between_dashes", [[(10 * i + 5, 9), (10 * i + 9, 9)] for i in range(3000)] + [[(0, 9), (9000, 9)]] + [[(10 * i + 5, 9), (10 * i + 9, 9)] for i in range(3000, 6000)] +
        [[(20000, 9), (70000, 9)], [(100, 9), (65000, 9)]])
    add("copies_10000", [[(5, 5), (25, 15)]] * 10000)
    add("nested", [[(500 - i, 3), (500 + i, 3)] for i in range(1, 150)])                       # every segment holds all the earlier ones: two pieces each
    rng = np.random.default_rng(5)
    lists = []
    for i in range(300):                                                      # zigzags in bands of their own: no two segments share a step
        x = np.cumsum(rng.integers(1, 9, int(rng.integers(2, 9)))) + int(rng.integers(0, 50))
        lists.append([(int(v), 10 * i + 7 * (k & 1)) for k, v in enumerate(x)])
    add("no_overlap_300", lists)
    return c


# (strokes, groups) -> (output strokes, origin), worked out by hand
HAND = [
    ([[(3, 3), (9, 6), (3, 3)]], None, [[(3, 3), (9, 6)]], [0]),
    ([[(10, 4), (20, 4)], [(0, 9), (0, 4), (30, 4), (30, 9)]], None, [[(10, 4), (20, 4)], [(0, 9), (0, 4), (10, 4)], [(20, 4), (30, 4), (30, 9)]], [0, 1, 1]),
    ([[(0, 4), (40, 4)], [(5, 4), (9, 4), (12, 4)], [(50, 4), (30, 4)], [(40, 4), (20, 4), (20, 8)]], None, [[(0, 4), (40, 4)], [(50, 4), (40, 4)], [(20, 4), (20, 8)]], [0, 2, 3]),
    ([[(10, 2), (20, 2), (0, 2)]], None, [[(10, 2), (20, 2)], [(10, 2), (0, 2)]], [0, 0]),
    ([[(0, 0), (8, 0)], [(8, 0), (0, 0)], [(0, 0), (8, 0)]], [0, 1, 0], [[(0, 0), (8, 0)], [(8, 0), (0, 0)]], [0, 1]),
    ([[(0, 0), (4, 0)], [(6, 0), (10, 0)], [(12, 0), (2, 0), (2, 5)]], None, [[(0, 0), (4, 0)], [(6, 0), (10, 0)], [(12, 0), (10, 0)], [(6, 0), (4, 0)], [(2, 0), (2, 5)]], [0, 1, 2, 2, 2]),
]


def random_drawing(seed):
    """up to 6 strokes of 2 - 6 points on a 3-, 5- or 9-wide grid, in two groups; the narrow grids are full of overlaps"""
    rng = np.random.default_rng(seed)
    w = (3, 5, 9)[seed % 3]
    lists = []
    for _ in range(int(rng.integers(1, 7))):
        P = [tuple(rng.integers(0, w, 2).tolist())]
        for _ in range(int(rng.integers(1, 6))):
            q = tuple(rng.integers(0, w, 2).tolist())
            while q == P[-1]:
                q = tuple(rng.integers(0, w, 2).tolist())
            P.append(q)
        lists.append(P)
    off, pts = strokes(lists)
    return off, pts, rng.integers(0, 2, len(lists)).astype(np.int32), 2


# ------------------------------------------------------------------ the tools
GRID_K, GRID_MM = 3, 5.0                            # gcode2stream: a 3 x 3 grid of closed squares of 5 mm = 200 steps at 40 steps per mm
GRID_STEPS_IN, GRID_STEPS_OUT = 36 * 200, 24 * 200


def tool_gcode(k=GRID_K, mm=GRID_MM):
    lines = ["G21 G90 M5"]
    for j in range(k):
        for i in range(k):
            s = square(20 + i * mm, 20 + j * mm, mm)
            lines += ["G0 X%g Y%g" % s[0], "M3"] + ["G1 X%g Y%g" % q for q in s[1:]] + ["M5"]
    return "\n".join(lines) + "\n"


TOOL_SVG_ARGS = ["--dedup", "--pen-colors", "#f00,#00f", "--scale", "1", "--margin-mm", "0"]


def tool_svg():
    """two red squares that share a border, two blue ones that share a border, and the red pair's right edge is the blue pair's left edge: two borders go, the
    one across the pens stays twice"""
    rects = [("#f00", 10, 10), ("#f00", 30, 10), ("#00f", 50, 10), ("#00f", 70, 10)]
    body = "".join(f'<rect x="{x}" y="{y}" width="20" height="20" fill="none" stroke="{c}"/>' for c, x, y in rects)
    return f'<svg xmlns="http://www.w3.org/2000/svg" width="210mm" height="297mm" viewBox="0 0 210 297">{body}</svg>'.encode()
