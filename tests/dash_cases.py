"""Drawings for the dash pass, each small: cases() -> {name: (off int64, pts int32 [total, 2], pattern int32 [n], phase int64 [n], pat_off int32, pat_val int64)};
random drawings of the kind the rule was tried on; and the two tool inputs.  The answers come from tests/dash_double.py.  Lengths are in u = 1/256 step."""
import numpy as np

TOP = 1 << 30
U = 256


def strokes(lists):
    off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
    return off, np.asarray([q for p in lists for q in p], np.int32).reshape(-1, 2)


def table(patterns):
    """(pat_off int32, pat_val int64) of a list of patterns, each a list of entries in u"""
    off = np.concatenate([[0], np.cumsum([len(p) for p in patterns])]).astype(np.int32)
    return off, np.asarray([e for p in patterns for e in p], np.int64)


def drawing(lists, pattern, phase, patterns):
    off, pts = strokes(lists)
    return (off, pts, np.asarray(pattern, np.int32), np.asarray(phase, np.int64)) + table(patterns)


def zigzag(n, x0=5, y0=5, seed=0):
    """n points, segments of one or two steps that go right and up or down in turn: a flattened curve, many vertices per dash"""
    rng = np.random.default_rng(seed)
    dx = rng.integers(1, 3, n - 1); dy = rng.integers(0, 3, n - 1) * np.where(np.arange(n - 1) % 2, -1, 1)
    x = x0 + np.concatenate([[0], np.cumsum(dx)]); y = y0 + 2 + np.concatenate([[0], np.cumsum(dy)])
    return list(zip(x.tolist(), (y - y.min() + y0).tolist()))


ON_OFF = [2 * U + U // 2, U + U // 4]                # 2.5 steps on, 1.25 off
LONG = [37 * U + 128, 11 * U + 77]                   # a dash over many vertices of a zigzag
M64 = [U + 37 * k for k in range(64)]                # 64 entries, all different
WHOLE = [3 * U, 2 * U, U, 4 * U]                     # whole steps
NEAR_TOP = [(1 << 40), (1 << 40) - 3]
POINT_COUNTS = (2, 63, 64, 65, 255, 256, 257, 1025)
STRIDE_LENGTHS = tuple(range(92, 101)) + tuple(range(185, 199))      # steps; with 2 on, 1 off: 31 .. 34 and 62 .. 66 dashes, 61 .. 66 and 123 .. 131 cut points


def cut_points(length_u, pat, phase):
    """the cut points of a 2-point stroke of length_u: the pattern's boundaries in (0, length_u], less a dash that would begin at the very end"""
    A = np.concatenate([[0], np.cumsum(pat)]).tolist()
    P, n, r = A[-1], 0, 0
    while r * P - phase <= length_u:
        n += sum(1 for t in range(len(pat)) if 0 < r * P + A[t] - phase <= length_u and not (t % 2 == 0 and r * P + A[t] - phase == length_u))
        r += 1
    return n


def cases():
    c = {}
    # 2-point strokes of 1 .. 110 steps: 0 .. 58 cut points each, every count on both sides of the hand-over from a thread to a wave
    c["two_points_every_count"] = drawing([[(3, k), (3 + k, k)] for k in range(1, 111)], [0] * 110, [0] * 110, [ON_OFF])
    c["two_points_slanted"] = drawing([[(3 + k, 2 * k), (3, 2 * k + k // 3)] for k in range(1, 111)], [0] * 110, [(7 * k) % 900 for k in range(110)], [ON_OFF])
    # a wave takes cut point e, e + 64, ..: strokes with 63, 64, 65 cut points and with 63, 64, 65 dashes (126 .. 130 cut points), where a lane's second turn
    # begins or does not; whole steps with a dash that ends on the last vertex or does not, and the same lengths entered a step and a bit into the pattern
    c["two_points_around_the_wave_stride"] = drawing([[(2, k), (2 + n, k)] for k, n in enumerate(STRIDE_LENGTHS)] + [[(300 + n, k), (300, k)] for k, n in enumerate(STRIDE_LENGTHS)],
                                                     [0] * (2 * len(STRIDE_LENGTHS)), [0] * len(STRIDE_LENGTHS) + [U + 77] * len(STRIDE_LENGTHS), [[2 * U, U]])
    c["a_thousand_dashes"] = drawing([[(0, 0), (3700, 411)], [(9, 9), (4, 5)], [(3750, 0), (0, 0)]], [0, -1, 0], [0, 0, 100], [ON_OFF])
    lists, pattern = [], []
    for k, n in enumerate(POINT_COUNTS):                                          # solid strokes between them: a stroke's head lies anywhere in a block
        lists += [zigzag(n, 5, 10 * k, seed=k), [(1, 10 * k), (2, 10 * k + 1), (1, 10 * k + 3)]]; pattern += [0, -1]
    c["many_points"] = drawing(lists, pattern, [0] * len(lists), [LONG])
    c["seventy_thousand_points"] = drawing([zigzag(70001, seed=9), [(0, 0), (5, 0)]], [0, 1], [5000, 0], [[300 * U + 9, 41 * U], ON_OFF])
    c["mixed_patterns"] = drawing([zigzag(40, seed=1), [(0, 0), (90, 0)], zigzag(90, 0, 30, seed=2), [(0, 50), (300, 260)], [(7, 7), (7, 90), (60, 90)], zigzag(300, 0, 70, seed=3)],
                                  [1, -1, 0, 1, 2, -1], [0, 0, 17, sum(M64) - 1, 3 * U, 0], [ON_OFF, M64, WHOLE])
    c["axis_parallel_whole_steps"] = drawing([[(0, 0), (23, 0), (23, 17), (4, 17), (4, 3)], [(50, 40), (50, 10)], [(10, 30), (20, 30), (30, 30)]], [0, 0, 0],
                                             [0, 4 * U, 9 * U], [WHOLE])
    c["phases"] = drawing([[(0, k), (40, k + 9)] for k in range(3)], [0] * 3, [0, sum(ON_OFF) - 1, U], [ON_OFF])      # 0, P - 1, and the first dash cut by the phase
    c["dash_longer_than_the_stroke"] = drawing([[(3, 3), (9, 7), (4, 12)], [(0, 0), (13, 0)]], [0, 0], [0, 0], [[200 * U, 300 * U]])
    c["wholly_in_a_gap"] = drawing([[(3, 3), (9, 7), (4, 12)], [(0, 0), (13, 0)], [(1, 1), (2, 5)]], [0, -1, 0], [50 * U, 0, 40 * U + 3], [[30 * U, 300 * U]])
    c["everything_vanishes"] = drawing([[(3, 3), (9, 7)]], [0], [50 * U], [[30 * U, 300 * U]])
    c["one_step_dashes_on_diagonals"] = drawing([[(0, 0), (60, 60)], [(60, 0), (0, 60)], [(0, 70), (40, 71)], [(5, 5), (6, 6), (7, 5), (8, 6), (9, 5)]], [0] * 4, [0, 100, 7, 300],
                                                [[U, U]])
    big = [[(0, 0), (TOP, TOP)], [(TOP, TOP), (0, 0)], [(0, TOP), (TOP, 0)], [(TOP, 0), (0, TOP)]]
    c["the_longest_segment"] = drawing(big + big, [0] * 4 + [1] * 4, [0, 12345, sum(NEAR_TOP) - 1, 1 << 39, 0, 77, 1 << 38, (1 << 39) + 563],
                                       [NEAR_TOP, [(1 << 38) + 7, U, 300, 1 << 39]])
    return c


def random_drawing(seed):
    """1 .. 5 strokes of 2 .. 8 points in a 50-step box, oblique or axis-parallel; 1 .. 3 patterns of 2, 4, 6 or 64 entries, of whole steps or not; every kind of phase"""
    rng = np.random.default_rng(seed)
    patterns = []
    for _ in range(int(rng.integers(1, 4))):
        m = int(rng.choice([2, 2, 4, 6, 64]))
        whole = rng.random() < 0.4
        patterns.append([U * int(rng.integers(1, 7)) if whole else int(rng.integers(U, U * int(rng.choice([2, 8, 40])) + 1)) for _ in range(m)])
    lists, pattern, phase = [], [], []
    for _ in range(int(rng.integers(1, 6))):
        k, axis = int(rng.integers(2, 9)), rng.random() < 0.4
        v = [(int(rng.integers(0, 41)), int(rng.integers(0, 41)))]
        while len(v) < k:
            if axis:
                d = int(rng.integers(1, 13)) * int(rng.choice([-1, 1]))
                q = (v[-1][0] + d, v[-1][1]) if rng.random() < 0.5 else (v[-1][0], v[-1][1] + d)
            else:
                q = (v[-1][0] + int(rng.integers(-9, 10)), v[-1][1] + int(rng.integers(-9, 10)))
            if q != v[-1] and min(q) >= 0:
                v.append(q)
        lists.append(v)
        q = int(rng.integers(-1, len(patterns)))
        pattern.append(q)
        P = sum(patterns[q]) if q >= 0 else 1
        phase.append([0, P - 1, int(rng.integers(0, P)), U * int(rng.integers(0, P // U + 1)) % P][int(rng.integers(0, 4))] if q >= 0 else 0)
    return drawing(lists, pattern, phase, patterns)


# ------------------------------------------------------------------ the tools' inputs
TOOL_GCODE = "\n".join(["G21 G90", "G0 X10 Y10", "M3", "G1 X60 Y10", "G1 X60 Y40", "M5", "G0 X10 Y50", "M3", "G1 X55.5 Y72.25", "M5", "G0 X5 Y5", "M3", "G1 X5.2 Y5", "M5"]) + "\n"
TOOL_GCODE_ARGS = ["--dash-mm", "2,1", "--dash-offset-mm", "0.5"]

TOOL_SVG = b"""<svg xmlns="http://www.w3.org/2000/svg" width="100mm" height="80mm" viewBox="0 0 100 80">
  <g stroke="black" fill="none" stroke-dasharray="4 2">
    <path d="M 10 10 L 90 10 L 90 40"/>
    <line x1="10" y1="20" x2="80" y2="35" style="stroke-dasharray: 1.5, 3, 5; stroke-dashoffset: 2"/>
    <circle cx="50" cy="55" r="15" stroke-dasharray="none"/>
    <g transform="scale(2)"><line x1="5" y1="35" x2="45" y2="38" stroke-dashoffset="-1"/></g>
  </g>
  <rect x="5" y="5" width="90" height="70" stroke="black" fill="none"/>
</svg>
"""
TOOL_SVG_ARGS = ["--dashes"]
