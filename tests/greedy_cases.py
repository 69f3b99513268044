"""Inputs of tests/test_gpu_greedy_paths.py, and a plain restatement of stage 07's greedy order that tests/test_oracle_greedy_paths.py holds to the oracle
and then reads the statistics from that the inputs were chosen for (coordinate-range flags, ties, closed contours entered, the kernel the host selects).

Polylines have 2 .. 5 points on a 25-px lattice, about 30 % of those with more than 3 points are closed, and they sit in a few clusters far apart:
equal distances occur all the time (index tie-break), and a cluster runs empty before the next one is reached."""
import numpy as np

LATTICE = 25
I16 = (-32768, 32767)           # beyond: NN_BEYOND_I16, no LDS store
B15 = (-16384, 16383)           # beyond: NN_BEYOND_15BIT, no grid kernel


def lattice_polys(seed, n, centres, spread=6, extra=()):
    """n polylines around `centres` (lattice offsets of up to `spread` steps), the polylines of `extra` (lists of points) replacing the last ones"""
    rng = np.random.default_rng(seed)
    centres = np.asarray(centres, np.int64)
    out = []
    for _ in range(n - len(extra)):
        c = centres[int(rng.integers(0, len(centres)))]
        m = int(rng.integers(2, 6))
        p = (c + rng.integers(-spread, spread + 1, (m, 2)) * LATTICE).astype(np.int32)
        if rng.random() < 0.3 and m > 3:
            p[-1] = p[0]
        out.append(p.reshape(-1, 1, 2))
    out += [np.asarray(e, np.int32).reshape(-1, 1, 2) for e in extra]
    return out


POS = [(1000, 1200), (9000, 2500), (15000, 15500), (3000, 14000)]                       # within 15 bits, lattice offsets included
NEG = [(-16000, -15900), (16000, 15500), (-3000, 9000), (8000, -16100)]                 # the whole signed 15-bit range: the grid kernel's origin shift
NEG16 = [(-32000, -30000), (32000, 31000), (-5000, 20000), (100, -32500)]               # the whole int16 range: the LDS store's signed shorts
BIG = [(1500 + 3200 * i, 1500 + 3100 * j) for i in range(5) for j in range(5)]          # 25 clusters for the 16 001 polylines

# name -> (seed, n, centres, spread, extra polylines, ORIP_NN_NOGRID, flags, kernel); kernel: "grid", "lds", "global256", "global1024"
CASES = {
    "n63": (1, 63, POS, 6, (), False, 0, "lds"),
    "n64": (2, 64, POS, 6, (), False, 0, "grid"),
    "n65": (3, 65, POS, 6, (), False, 0, "grid"),
    "n70_x20000": (4, 70, POS, 6, ([[20000, 3000], [19950, 3025]],), False, 2, "global256"),
    "n70_y-20000": (5, 70, POS, 6, ([[4000, 4000], [4025, 4050], [4000, -20000]],), False, 2, "global256"),
    "n40_40000": (6, 40, POS, 6, ([[40000, 5000], [39975, 5000]],), False, 3, "global256"),
    "n70_40000": (7, 70, POS, 6, ([[2000, 2025], [2000, 40000]],), False, 3, "global256"),
    "n70_negative": (8, 70, NEG, 6, (), False, 0, "grid"),
    "n40_negative": (9, 40, NEG16, 6, (), False, 2, "lds"),
    "n200_nogrid": (10, 200, POS, 6, (), True, 0, "lds"),
    "n16001": (11, 16001, BIG, 40, (), False, 0, "global1024"),
}
SMALL = [k for k, v in CASES.items() if v[1] <= 200]


def polys_of(name):
    seed, n, centres, spread, extra, _, _, _ = CASES[name]
    return lattice_polys(seed, n, centres, spread, extra)


def ends07(polys):
    """start, end under rule07 (a closed contour ends at its second-to-last point and is entered at its start only), closed"""
    P = [np.asarray(p).reshape(-1, 2).astype(np.int64) for p in polys]
    closed = np.array([len(p) >= 2 and bool((p[0] == p[-1]).all()) for p in P])
    start = np.array([p[0] for p in P])
    end = np.array([p[-2] if c else p[-1] for p, c in zip(P, closed)])
    return start, end, closed


def range_flags(polys):
    """k_argmax_feat's coordinate-range flags over the end points"""
    s, e, _ = ends07(polys)
    xy = np.concatenate([s, e])
    return (1 if (xy < I16[0]).any() or (xy > I16[1]).any() else 0) | (2 if (xy < B15[0]).any() or (xy > B15[1]).any() else 0)


def selected_kernel(n, flags, nogrid):
    """the host logic of vreorder: which of the enqueued kernels runs"""
    G = 8
    while G < 128 and (G + 8) * (G + 8) <= 4 * n and n * 12 + ((G + 8) * (G + 8) + 1) * 4 + 64 <= 158 * 1024:
        G += 8
    grid_ok = 64 <= n <= 16000 and n * 12 + (G * G + 1) * 4 + 64 <= 158 * 1024 and not nogrid
    lds_ok = n <= 16000
    if grid_ok:
        return "grid" if flags == 0 else "global256"
    if lds_ok:
        return "lds" if not flags & 1 else "global256"
    return "global1024"


def greedy07(polys, seed_index):
    """the greedy order from `seed_index` on: [(index, flip)], the number of steps whose smallest distance is shared by different polylines, and the
    number of closed contours entered.  Distances are float32 sums of float32 squares, the smallest (distance, index) wins, a polyline is read
    backwards when its end is strictly nearer."""
    start, end, closed = ends07(polys)
    sf, ef = start.astype(np.float32), end.astype(np.float32)
    n = len(polys)
    used = np.zeros(n, bool); used[seed_index] = True
    order = [(seed_index, False)]
    cur = start[seed_index] if closed[seed_index] else end[seed_index]
    ties = entered = 0
    for _ in range(1, n):
        c = cur.astype(np.float32)
        ds = ((sf - c) ** 2).sum(1, dtype=np.float32); de = ((ef - c) ** 2).sum(1, dtype=np.float32)
        v = np.where(closed | (ds <= de), ds, de)
        v[used] = np.inf
        i = int(np.argmin(v))                      # the first of equal minima
        ties += int((v == v[i]).sum() > 1)
        flip = bool(not closed[i] and not ds[i] <= de[i])
        entered += int(closed[i])
        used[i] = True; order.append((i, flip))
        cur = start[i] if closed[i] or flip else end[i]
    return order, ties, entered


def apply_order(polys, order):
    return [np.asarray(polys[i]).reshape(-1, 2)[::-1] if flip else np.asarray(polys[i]).reshape(-1, 2) for i, flip in order]
