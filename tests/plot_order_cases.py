"""TEST INFRASTRUCTURE: named cases for stage 12 (orip_plot_order, csrc/vector.hip) and an exact restatement of the stage to reason about them.

cases() returns {name: (lines, taps, R)}: lines a list of int32 [n, 1, 2] arrays, taps a list of (x, y), R the insert radius.  No GPU import.
tests/test_oracle_plot_order_cases.py runs them through the oracle and asserts that every case holds what its name claims;
tests/test_gpu_plot_order_cases.py runs them through both device kernels and compares raw op rows.

model() is the same greedy on exact integer d^2 with numpy (candidate order: line 0 start, line 0 end, line 1 start, ..., then the taps; the first minimum
wins), and it keeps a trace of every choice and every drained tap.  With wrap=True the distance is taken mod 2^32 before it is compared, which is what a key
of (d^2 << 32) | index in 64 bits does: the wide cases are placed so that this changes the answer."""
import math

import numpy as np

R0 = 80.0
LDS_LIMIT = 150 * 1024          # the wave kernel's lists: 17 bytes a line, 9 a tap, 64 spare (orip_plot_order)
COORD_MAX = 1 << 24             # the stage's contract (include/orip.h)


def line(*pts):
    return np.array(pts, np.int32).reshape(-1, 1, 2)


def lds_bytes(nl, nt):
    return 17 * nl + 9 * nt + 64


# ---------------------------------------------------------------------------------------------- the model
def model(lines, taps, R, wrap=False):
    """-> (rows int32 [n, 5], trace).  trace entries:
    {"ev": "first", "k", "flip", "same_len": lines as long as the chosen one}
    {"ev": "pick", "idx": candidate index (2 k, 2 k + 1, 2 nl + t), "ties": candidates at the same least distance, "d2", "nops"}
    {"ev": "drain", "run": number of the pass, "t", "offset": t minus the pass's cursor, "d2", "from": the position the distance was taken from, "nops"}"""
    nl, nt = len(lines), len(taps)
    P = [np.asarray(p, np.int64).reshape(-1, 2) for p in lines]
    ends = np.array([[p[0, 0], p[0, 1], p[-1, 0], p[-1, 1]] if len(p) else [0, 0, 0, 0] for p in P], np.int64).reshape(nl, 4)
    valid = np.array([len(p) >= 2 for p in P], bool)
    T = np.asarray(list(taps), np.int64).reshape(nt, 2)
    cx = np.concatenate([ends[:, [0, 2]].reshape(-1), T[:, 0]]); cy = np.concatenate([ends[:, [1, 3]].reshape(-1), T[:, 1]])
    alive = np.concatenate([np.repeat(valid, 2), np.ones(nt, bool)])
    rows, trace, pos, runs = [], [], (0, 0), [0]

    def d2_from(p):
        return (cx - p[0]) ** 2 + (cy - p[1]) ** 2

    def drain():
        nonlocal pos
        cursor, run = 0, runs[0]
        runs[0] += 1
        while cursor < nt:
            d2 = d2_from(pos)[2 * nl + cursor:]
            hit = alive[2 * nl + cursor:] & (np.sqrt(d2.astype(np.float64)) <= R)
            if not hit.any():
                break
            o = int(np.argmax(hit)); t = cursor + o
            trace.append({"ev": "drain", "run": run, "t": t, "offset": o, "d2": int(d2[o]), "from": pos, "nops": len(rows)})
            rows.append((1, -1, 0, int(T[t, 0]), int(T[t, 1]))); alive[2 * nl + t] = False
            pos = (int(T[t, 0]), int(T[t, 1])); cursor = t + 1

    def take_line(k, flip):
        nonlocal pos
        rows.append((0, k, flip, 0, 0)); alive[2 * k] = alive[2 * k + 1] = False
        pos = (int(ends[k, 0]), int(ends[k, 1])) if flip else (int(ends[k, 2]), int(ends[k, 3]))
        drain()

    if valid.any():
        ln = np.array([np.hypot(*np.diff(p.astype(np.float32), axis=0).T).sum(dtype=np.float32) if len(p) >= 2 else -1 for p in P], np.float32)
        k = int(np.argmax(ln))
        flip = int(ends[k, 2] ** 2 + ends[k, 3] ** 2 < ends[k, 0] ** 2 + ends[k, 1] ** 2)
        trace.append({"ev": "first", "k": k, "flip": flip, "same_len": [int(i) for i in np.nonzero(ln == ln[k])[0]]})
        take_line(k, flip)
    while alive.any():
        d2 = d2_from(pos)
        key = np.where(alive, (d2 & 0xffffffff) if wrap else d2, np.iinfo(np.int64).max)
        idx = int(np.argmin(key))
        trace.append({"ev": "pick", "idx": idx, "ties": [int(i) for i in np.nonzero(key == key[idx])[0]], "d2": int(d2[idx]), "nops": len(rows)})
        if idx < 2 * nl:
            take_line(idx >> 1, idx & 1)
        else:
            t = idx - 2 * nl
            rows.append((1, -1, 0, int(T[t, 0]), int(T[t, 1]))); alive[idx] = False; pos = (int(T[t, 0]), int(T[t, 1]))
    return np.array(rows, np.int32).reshape(-1, 5), trace


# ---------------------------------------------------------------------------------------------- A.1 the ring and the totals
TOTALS = [1, 2, 63, 64, 65, 127, 128, 129, 192]


def _rand_lines(rng, n, span=3000, lo=0):
    return [line(*rng.integers(lo, span, (2, 2))) for _ in range(n)]


def _rand_taps(rng, n, span=3000, lo=0):
    return [(int(x), int(y)) for x, y in rng.integers(lo, span, (n, 2))]


def _groups(total, nl):
    """op numbers at which the lines come when line i is followed by its run of taps: tap j belongs to line j % nl"""
    nt = total - nl
    sizes = [1 + (nt // nl) + (1 if i < nt % nl else 0) for i in range(nl)]
    return [sum(sizes[:i]) for i in range(nl)]


def mixed_total(total):
    """lines 1000 px apart along y = 0, each followed by a run of taps 10 px apart behind its end, so that every line's pass drains a whole run: nl is the first
    count from total / 9 up with which the ops on either side of every multiple of 64 are taps of one run"""
    nl = next(n for n in range(max(1, total // 9), total) if not any(m - 1 in _groups(total, n) or (m < total and m in _groups(total, n)) for m in range(64, total + 1, 64)))
    nt = total - nl
    lines = [line((1000 * i, 0), (1000 * i + (501 if i == 0 else 500), 0)) for i in range(nl)]
    taps = [(1000 * (j % nl) + 500 + 10 * (j // nl + 1), 5) for j in range(nt)]
    return lines, taps


def total_cases():
    c = {}
    for n in TOTALS:
        rng = np.random.default_rng(1200 + n)
        c["total_%d_lines" % n] = (_rand_lines(rng, n), [], R0)
        c["total_%d_taps" % n] = ([], _rand_taps(rng, n), R0)
        if n >= 2:
            c["total_%d_mixed" % n] = mixed_total(n) + (R0,)
    return c


# ---------------------------------------------------------------------------------------------- A.2 the insert radius
# R -> lattice vectors of exactly that length (80.5: the last d^2 inside, 6480 = 72^2 + 36^2; its neighbour below is (80, 9), d^2 = 6481 > 80.5^2 = 6480.25)
RADIUS_VECTORS = {80.0: [(48, 64), (64, 48), (80, 0)], 81.0: [(81, 0)], 200.0: [(120, 160), (56, 192)], 1000.0: [(600, 800), (280, 960), (352, 936)], 80.5: [(72, 36)]}
RADIUS_OUTSIDE = {80.5: lambda v: (80, 9)}          # every other radius: the vector one unit further out in y, e.g. (80, 1) for (80, 0)
SCENE_STEP = 6000


def radius_scene(i, v, q):
    """line A ends at E; tap Q = E + q (just outside R, lower index) and tap P = E + v (exactly at R, or the last lattice distance inside); line B starts 10 px
    from E and ends towards the next scene, whose A is the nearest thing from there.  With P drained the cursor moves to P and Q (next to it) comes before B;
    with P left, B (10 px) comes first.  The first scene's A is the longest line of the case"""
    ex, ey = SCENE_STEP * i + 4000, 3000
    A = line((ex - (3000 if i == 0 else 300), ey), (ex, ey))
    B = line((ex, ey - 10), (ex + 2400, ey - 10))
    return [A, B], [(ex + q[0], ey + q[1]), (ex + v[0], ey + v[1])], (ex, ey)


def radius_case(R):
    lines, taps = [], []
    for i, v in enumerate(RADIUS_VECTORS[R]):
        q = RADIUS_OUTSIDE[R](v) if R in RADIUS_OUTSIDE else (v[0], v[1] + 1)
        l, t, _ = radius_scene(i, v, q)
        lines += l; taps += t
    return lines, taps, R


CHAIN_E = (1000, 1000)


def chain_case():
    """taps 70 px apart behind the line's end: only the first is within R of the end, each next one only of the tap before it"""
    ex, ey = CHAIN_E
    return [line((100, ey), (ex, ey)), line((ex, ey - 30), (ex, ey - 900))], [(ex + 70 * (j + 1), ey) for j in range(5)], R0


def forward_only_case():
    """tap 0 is 140 px from the line's end, tap 1 is 70 px: the pass drains tap 1, which brings tap 0 within R of the cursor, but the pass does not go back.
    Line B starts 30 px from tap 1, so the nearest search takes B before it comes to tap 0"""
    ex, ey = CHAIN_E
    return [line((100, ey), (ex, ey)), line((ex + 70, ey + 30), (ex + 70, ey + 900))], [(ex + 140, ey), (ex + 70, ey)], R0


CHUNK_OFFSETS = [0, 63, 64, 1023, 1024, 1100]


def chunk_case():
    """hits 50 px apart behind the line's end, each CHUNK_OFFSETS[j] taps after the cursor the hit before it left; every tap in between is alive and 20 000 px away"""
    ex, ey = 500, 10
    taps, hits = [], []
    for j, o in enumerate(CHUNK_OFFSETS):
        taps += [(20000 + 3 * (len(taps) + i), 20000 + (i % 7)) for i in range(o)]
        hits.append(len(taps)); taps.append((ex + 50 * (j + 1), ey))
    taps += [(20000 + 3 * (len(taps) + i), 20000 + (i % 7)) for i in range(10)]
    return [line((10, ey), (ex, ey))], taps, R0, hits


# ---------------------------------------------------------------------------------------------- A.3 ties, A.4 the first op, A.5 degenerate and signed
A0 = line((0, 0), (1000, 0))          # the longest line of the small cases below: drawn first, not flipped, the cursor is then at (1000, 0)

# name -> (lines, taps, R, the rows worked by hand)
HAND = {
    # B's start and end are both 50 px from A's end: the start wins; C is closed and 50 px from B's end: entered unflipped
    "tie_start_end": ([A0, line((1000, 50), (1200, 50), (1000, -50)), line((1000, -100), (1100, -100), (1000, -100))], [], R0,
                      [(0, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 2, 0, 0, 0)]),
    # the end of line 1 and the start of line 2 are both 40 px from A's end: line 1 wins, flipped
    "tie_end_j_start_k": ([A0, line((2000, 40), (1000, 40)), line((1000, -40), (900, -40))], [], R0, [(0, 0, 0, 0, 0), (0, 1, 1, 0, 0), (0, 2, 0, 0, 0)]),
    # a line start (100, 0) and a tap (60, 80) both 100 px from A's end: the line wins; the tap follows from (1900, 0)
    "tie_line_tap": ([A0, line((1100, 0), (1900, 0))], [(1060, 80)], R0, [(0, 0, 0, 0, 0), (0, 1, 0, 0, 0), (1, -1, 0, 1060, 80)]),
    # two taps 100 px from A's end: the lower index wins
    "tie_two_taps": ([A0], [(1000, -100), (1000, 100)], R0, [(0, 0, 0, 0, 0), (1, -1, 0, 1000, -100), (1, -1, 0, 1000, 100)]),
    # taps only, no pass ever runs: from (100, 100) the vectors (5, 0) and (3, 4) are both d^2 = 25, the lower index wins
    "tie_5_0_3_4": ([], [(100, 100), (105, 100), (103, 104)], R0, [(1, -1, 0, 100, 100), (1, -1, 0, 105, 100), (1, -1, 0, 103, 104)]),
    "tie_3_4_5_0": ([], [(100, 100), (103, 104), (105, 100)], R0, [(1, -1, 0, 100, 100), (1, -1, 0, 103, 104), (1, -1, 0, 105, 100)]),
    # d^2 = 625 three ways, (25, 0), (15, 20) and (7, 24) from (100, 100): the lowest index wins, whichever vector it holds
    "tie_25_15_7": ([], [(100, 100), (125, 100), (115, 120), (107, 124)], R0, [(1, -1, 0, 100, 100), (1, -1, 0, 125, 100), (1, -1, 0, 115, 120), (1, -1, 0, 107, 124)]),
    "tie_7_15_25": ([], [(100, 100), (107, 124), (115, 120), (125, 100)], R0, [(1, -1, 0, 100, 100), (1, -1, 0, 107, 124), (1, -1, 0, 115, 120), (1, -1, 0, 125, 100)]),
    # lines 1 and 2 are the same line: index 1 first, unflipped, then index 2 from the far end, flipped; the two equal taps are two ops
    "duplicates": ([A0, line((1100, 0), (1200, 0)), line((1100, 0), (1200, 0))], [(5000, 5000), (5000, 5000)], R0,
                   [(0, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 2, 1, 0, 0), (1, -1, 0, 5000, 5000), (1, -1, 0, 5000, 5000)]),
    # three lines of float32 length 5: the first index is the first op; its start is on the origin, so it is not flipped
    "first_equal_len": ([line((0, 0), (5, 0)), line((0, 0), (3, 4)), line((10, 10), (10, 15))], [], R0, [(0, 0, 0, 0, 0), (0, 1, 1, 0, 0), (0, 2, 0, 0, 0)]),
    # both ends 50 px from the origin: strict <, not flipped
    "first_ends_equal": ([line((30, 40), (100, 100), (40, 30))], [], R0, [(0, 0, 0, 0, 0)]),
    "first_end_nearer": ([line((500, 500), (10, 10))], [], R0, [(0, 0, 1, 0, 0)]),
    # taps only: (3, 4) and (5, 0) equally near the origin, the lower index first; then (0, 5) at d^2 10 from (3, 4) before (5, 0) at 20
    "first_taps_tie": ([], [(3, 4), (5, 0), (0, 5)], R0, [(1, -1, 0, 3, 4), (1, -1, 0, 0, 5), (1, -1, 0, 5, 0)]),
    "first_tap_on_origin": ([], [(7, 7), (0, 0), (3, 3)], R0, [(1, -1, 0, 0, 0), (1, -1, 0, 3, 3), (1, -1, 0, 7, 7)]),
    "empty": ([], [], R0, []),
    # a one-point line is no op (12:95-96): line 1 never shows, although it lies on A's end
    "one_point_line": ([A0, line((1000, 0)), line((1300, 0), (1400, 0))], [(3000, 0)], R0, [(0, 0, 0, 0, 0), (0, 2, 0, 0, 0), (1, -1, 0, 3000, 0)]),
    # no line of two points: the first op is the tap nearest to the origin, as with no lines at all
    "one_point_lines_only": ([line((1, 1)), line((2000, 2000))], [(500, 0), (300, 0)], R0, [(1, -1, 0, 300, 0), (1, -1, 0, 500, 0)]),
    "one_point_alone": ([line((5, 5))], [], R0, []),
    # the one-point line and the two-point line of length 0 both have length 0: only the second is a line
    "one_point_zero_length": ([line((5, 5)), line((9, 9), (9, 9))], [], R0, [(0, 1, 0, 0, 0)]),
}

LONG_POINTS = 300          # > ORIP_LONG_POLY = 192 (csrc/vec_common.h): the line's length comes from the block-per-polyline kernel


def first_long_case():
    """the staircase of 300 points has length 299; line 0 (length 298) would be first if the long line's length came out short"""
    stair = [(100 + (i + 1) // 2, 100 + i // 2) for i in range(LONG_POINTS)]
    return [line((0, 0), (298, 0)), line(*stair), line((400, 400), (400, 500))], [(260, 250)], R0


def signed_case():
    rng = np.random.default_rng(1205)
    return _rand_lines(rng, 40, 3000, -3000), _rand_taps(rng, 90, 3000, -3000), R0


# ---------------------------------------------------------------------------------------------- A.6 list sizes at the LDS limit
LDS_CASES = {"lds_over": (8800, 438), "lds_under": (8800, 437)}


def lds_case(name):
    nl, nt = LDS_CASES[name]
    rng = np.random.default_rng(1206)
    return _rand_lines(rng, nl, 12000), _rand_taps(rng, nt, 12000), R0


# ---------------------------------------------------------------------------------------------- A.7 wide
def wide_case(S, signed=False):
    """line 0 runs from the far corner to (10, 0) and is drawn flipped, so the cursor stands at the far corner (S, S).  From there: candidates a few thousand px
    away, and candidates whose d^2 is a multiple of 2^32 (S, 65536 and 2 * 65536 px away along an axis, and across the diagonal when signed), which a wrapped
    key takes for distance 0"""
    lo = -S if signed else 0
    lines = [line((S, S), (10, 0)),
             line((S - 3000, S), (S - 3000, S - 500)),              # near
             line((S - 65536, S - 7), (S - 65536, S)),              # its end is 65536 px from the corner
             line((lo, S), (lo + 40, S))]                           # its start is S (2 S when signed) px from the corner
    taps = [(S, lo), (S - 2000, S), (S - 131072, S), (S, S - 1500), (lo, lo)]
    return lines, taps, R0


WIDE = {"wide_two_taps": ([], [(70000, 0), (30000, 0)], R0),
        "wide_2p17": wide_case(1 << 17), "wide_2p20": wide_case(1 << 20), "wide_2p24": wide_case(1 << 24), "wide_pm_2p24": wide_case(1 << 24, signed=True),
        # three taps 100 000 px from the origin (d^2 = 10^10, past 2^32): the lowest index wins, then the nearer of the other two
        # (from the first, (0, 100000) is 4.0e9 away in d^2 and (100000, 0) 8.0e9, which wraps to 3.7e9)
        "wide_tie": ([], [(60000, 80000), (100000, 0), (0, 100000)], R0)}
# refused: one coordinate one past the contract, in a tap, in a line's start and in a line's end, on either side
REFUSED = {"tap_x": ([A0], [(COORD_MAX + 1, 0)]), "tap_y_neg": ([A0], [(5, -COORD_MAX - 1)]), "line_start": ([A0, line((-COORD_MAX - 1, 3), (5, 5))], []),
           "line_end": ([A0, line((5, 5), (7, COORD_MAX + 1))], [(9, 9)])}


def small_cases():
    """every case but the two at the LDS limit"""
    c = total_cases()
    for R in RADIUS_VECTORS:
        c["radius_%g" % R] = radius_case(R)
    c["chain"] = chain_case(); c["forward_only"] = forward_only_case(); c["chunks"] = chunk_case()[:3]
    for n, v in HAND.items():
        c[n] = v[:3]
    c["first_long_poly"] = first_long_case(); c["signed"] = signed_case()
    c.update(WIDE)
    return c


def cases():
    c = small_cases()
    for n in LDS_CASES:
        c[n] = lds_case(n)
    return c
