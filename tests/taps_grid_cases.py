"""TEST INFRASTRUCTURE: named cases for stage 10's tap filter with its cell hash (k_taps_grid, csrc/vector10.hip), a plain restatement of the sequential rule that
says for every candidate why it went, and the kernel's LDS rule.

cases() returns {name: case} in the form of cross_cases.py: one layer, candidates given as the layer's taps (tap_diam = 0: no line becomes a tap), D_lines = 1 (a
kept line forbids exactly its own vertices, so a `domino` of two pixels puts one chosen pixel into the raster before the layer's taps are filtered).
tests/test_oracle_taps_grid.py shows with the oracle and verdicts() what every case reaches; tests/test_gpu_taps_grid.py runs them on the device.  No GPU import.

The kernel's cells are r px a side (max(r, 1)), whatever the canvas.  The radii are 1, 3 and 70: with 70 a cell is wider than the smallest canvas (64 x 64), every
candidate inside lies in one cell and each is within r of most others.

The chains have 200 candidates where the largest canvas (256 x 256) holds them: at r = 1, the chain at exactly r along a row, the chain just beyond r along the
diagonal (200 steps of (1, 1), d^2 = r^2 + 1; along a row at r + 1 = 2 px only 128 fit, which is a case too).  A candidate off the canvas is accepted whatever
lies near it, so a chain cannot run on past the canvas edge: at r = 3 the chains have the 86 (at r) and 64 (at r + 1) candidates that fit into 256 px, at
r = 70 the 4 that fit."""
import numpy as np

import cross_cases as X

RADII = [1, 3, 70]
COUNTS = [1, 63, 64, 65, 129]
LDS_LIMIT = 150 * 1024
OUT, ACC = 0, 2
# lattice vectors of length exactly r, and one with d^2 = r^2 + 1
ON_CIRCLE = {1: [(1, 0), (0, 1)], 3: [(3, 0), (0, 3)], 70: [(70, 0), (42, 56), (56, 42)]}
JUST_OUTSIDE = {1: (1, 1), 3: (3, 1), 70: (70, 1)}


def lds_bytes(n):
    """TapsGridLds: int2 cand[n], int next[n], int head[slots], u8 st[n], slots the power of two in (n / 2, n], at least 64"""
    slots = 64
    while slots * 2 <= n:
        slots *= 2
    return (13 * n + 4 * slots + 15) & ~15


def cell(p, r):
    return (p[0] // max(r, 1), p[1] // max(r, 1))


def verdicts(cands, forb, r):
    """the sequential rule, candidate by candidate -> [(state, why)]: state ACC / OUT, why "off" (off the canvas), "free", "raster" or the index of the
    first accepted candidate within r"""
    H, W = forb.shape
    out, acc = [], []
    for i, (x, y) in enumerate(cands):
        if not (0 <= x < W and 0 <= y < H):
            out.append((ACC, "off")); acc.append(i); continue
        if forb[y, x]:
            out.append((OUT, "raster")); continue
        hit = next((j for j in acc if (cands[j][0] - x) ** 2 + (cands[j][1] - y) ** 2 <= r * r), None)
        if hit is None:
            out.append((ACC, "free")); acc.append(i)
        else:
            out.append((OUT, hit))
    return out


def depth(cands, forb, r):
    """the number of rounds the kernel needs at least: the longest chain i_1 < i_2 < ... of candidates that passed the raster, each within r of the one before"""
    H, W = forb.shape
    live = [i for i, (x, y) in enumerate(cands) if not (0 <= x < W and 0 <= y < H) or not forb[y, x]]
    d = {}
    for i in live:
        inside = 0 <= cands[i][0] < W and 0 <= cands[i][1] < H
        d[i] = 1 + max([d[j] for j in live if j < i and inside and (cands[j][0] - cands[i][0]) ** 2 + (cands[j][1] - cands[i][1]) ** 2 <= r * r], default=0)
    return max(d.values(), default=0)


def tcase(name, W, H, r, cands, lines=()):
    return X.case(name, W, H, [([X.P(l) for l in lines], [(int(x), int(y)) for x, y in cands])], D_taps=2.0 * r)


def radius_of(c):
    return X.rad_taps(X.prm_of(c))


def forb_of(c):
    """the raster the layer's taps are filtered against: the vertices of the layer's own lines"""
    forb = np.zeros((c["H"], c["W"]), np.uint8)
    for l in c["layers"][0][0]:
        for x, y in np.asarray(l).reshape(-1, 2):
            forb[y, x] = 255
    return forb


def _rand(n, seed, lo, hi):
    rng = np.random.default_rng(seed)
    return [(int(x), int(y)) for x, y in rng.integers(lo, hi, (n, 2))]


def count_case(n, r):
    """n random candidates on and around the 64 x 64 canvas (a tenth of them off it)"""
    return tcase("count_%d_r%d" % (n, r), 64, 64, r, _rand(n, 1400 + n + r, -4, 68))


def boundary_case(r):
    """for every lattice vector v of length exactly r a pair (p, p + v), the second refused, and a pair (p, p + w) with |w|^2 = r^2 + 1, both accepted; the
    pairs lie 20 px apart along the diagonal.  At r = 70 every pair is a case of its own: the canvas holds no two of them more than r apart"""
    vs = [(v, False) for v in ON_CIRCLE[r]] + [(JUST_OUTSIDE[r], True)]
    if r == 70:
        return [tcase("boundary_r70_%d" % i, 256, 256, r, [(20, 30), (20 + v[0], 30 + v[1])]) for i, (v, _) in enumerate(vs)]
    cands = []
    for i, (v, _) in enumerate(vs):
        p = (10 + 20 * i, 10 + 20 * i)
        cands += [p, (p[0] + v[0], p[1] + v[1])]
    return [tcase("boundary_r%d" % r, 256, 256, r, cands)]


def chain_len(r, step):
    return min(200, 255 // step + 1)


def chain_case(r, step):
    """collinear candidates `step` px apart along y = 100, in order"""
    n = chain_len(r, step)
    return tcase("chain_r%d_step%d" % (r, step), 256, 256, r, [(step * i, 100) for i in range(n)])


def diag_chain_case():
    """200 candidates along the diagonal at r = 1: each sqrt(2) from the one before, d^2 = r^2 + 1"""
    return tcase("chain_r1_diag", 256, 256, 1, [(20 + i, 30 + i) for i in range(200)])


def repeated_case(r):
    return tcase("repeated_r%d" % r, 64, 64, r, [(33, 21)] * 100)


def full_cell_case(r):
    """80 candidates, every one in the cell of (2 r, 3 r)"""
    rng = np.random.default_rng(1450 + r)
    return tcase("full_cell_r%d" % r, 256, 256, r, [(2 * r + int(a), 3 * r + int(b)) for a, b in rng.integers(0, r, (80, 2))])


def borders_case(r):
    """candidates on both sides of the cell borders (x or y a multiple of r, and one less), around a crossing of borders, and in the four corner cells of the canvas"""
    W = H = 64 if r < 70 else 256
    k = (W // 2) // r * r if r < 70 else 140
    near = [(k + a, k + b) for a in (-1, 0) for b in (-1, 0)] + [(k - 1, k + r - 1), (k + r - 1, k - 1), (k, k - r), (k - r, k)]
    corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (1, 1), (W - 2, 1), (1, H - 2), (W - 2, H - 2)]
    rng = np.random.default_rng(1460 + r)
    order = rng.permutation(len(near) + len(corners))
    both = near + corners
    return tcase("borders_r%d" % r, W, H, r, [both[i] for i in order])


def off_canvas_case(r):
    """candidates off the canvas on all four sides (negative, and >= W, >= H), twice each, followed by candidates inside within r of them and others beyond r"""
    W = H = 64 if r < 70 else 256
    off = [(-1, 20), (-1, 20), (W, 40), (W, 40), (30, -1), (30, H), (-r, -r), (W + r - 1, H + r - 1)]
    inside = [(0, 20), (r, 20), (W - 1, 40), (W - r, 40), (W - r - 1, 41), (30, 0), (30, r), (30, H - 1), (30, H - 1 - r), (0, 0), (W - 1, H - 1), (32, 32)]
    return tcase("off_canvas_r%d" % r, W, H, r, off[:4] + inside[:5] + off[4:] + inside[5:])


def raster_case(r):
    """a is accepted; b, r px from it on the raster (the layer's own domino), goes; c is within r of b only, and b blocks nothing: accepted.
    d is accepted; e, on the raster, r px from d, stands between d and f in the order; f is exactly r from d: refused by d"""
    dom = [[(100 + r, 200), (100 + r, 201)], [(20 + r, 30), (20 + r, 31)]]
    cands = [(100, 200), (100 + r, 200), (100 + 2 * r, 200), (20, 30), (20 + r, 30), (20, 30 + r)]
    return tcase("raster_r%d" % r, 256, 256, r, cands, dom)


def empty_case():
    return tcase("empty", 64, 64, 3, [])


LDS_N = {"lds_under": 9294, "lds_over": 9295}


def lds_case(name):
    """random candidates on a canvas of 256 x 256 at r = 3, one short of and one past the one-workgroup kernel's LDS: the size rule alone chooses the kernel"""
    return tcase(name, 256, 256, 3, _rand(LDS_N[name], 1470, -3, 259))


def cases():
    c = {}
    for r in RADII:
        for n in COUNTS:
            k = count_case(n, r); c[k["name"]] = k
        for k in boundary_case(r):
            c[k["name"]] = k
        for k in (chain_case(r, r), chain_case(r, r + 1), repeated_case(r), full_cell_case(r), borders_case(r), off_canvas_case(r), raster_case(r)):
            c[k["name"]] = k
    c["empty"] = empty_case(); c["chain_r1_diag"] = diag_chain_case()
    return c
