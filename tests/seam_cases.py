"""TEST INFRASTRUCTURE: inputs of the --loop-start tests, shared by the host and the GPU files.  A case is (off int64 [n + 1], pts int32 [total, 2], order
int32 [n] or None, rev bool [n] or None, start).  The sequence is any permutation: the rule does not ask for the greedy order."""
import numpy as np

TOP = 1 << 30
HAND_OVER = 1 << 20              # SM_HAND_OVER of csrc/gcode_seam.hip: pairs of one layer from which it gets blocks of its own


def pack(strokes, order=None, rev=None, start=(0, 0)):
    lens = [len(s) for s in strokes]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pts = np.concatenate([np.asarray(s, np.int64).reshape(-1, 2) for s in strokes]).astype(np.int32) if strokes else np.zeros((0, 2), np.int32)
    return (off, pts, None if order is None else np.asarray(order, np.int32), None if rev is None else np.asarray(rev, bool), start)


def ring(cx, cy, r, m, turn=0.0):
    """a closed stroke of m ring vertices (m + 1 points) on a circle; r is large enough for m that no two neighbours share a grid point"""
    a = turn + 2.0 * np.pi * np.arange(m) / m
    p = np.stack([np.rint(cx + r * np.cos(a)), np.rint(cy + r * np.sin(a))], 1).astype(np.int64)
    assert (np.abs(np.diff(np.concatenate([p, p[:1]]), axis=0)).max(1) > 0).all()
    return np.concatenate([p, p[:1]])


def square(x, y, s):
    return np.array([[x, y], [x + s, y], [x + s, y + s], [x, y + s], [x, y]], np.int64)


def line(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y1]], np.int64)


def radius(m):
    return max(4, m)             # a chord of 2 r sin(pi / m) >= 2 steps or so


def tiny(seed):
    """1 - 4 strokes on coordinates 0 .. 5: rings of 3 - 4 vertices, open strokes of 2 - 4 points (A, B, A among them), a seeded sequence"""
    rng = np.random.default_rng(seed)
    strokes = []
    for _ in range(int(rng.integers(1, 5))):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            strokes.append(rng.integers(0, 6, (int(rng.integers(2, 5)), 2)))
        elif kind == 1:
            a, b = rng.integers(0, 6, (2, 2))
            strokes.append(np.array([a, b, a]))
        else:
            p = rng.integers(0, 6, (int(rng.integers(3, 5)), 2))
            strokes.append(np.concatenate([p, p[:1]]))
    n = len(strokes)
    return pack(strokes, rng.permutation(n), rng.integers(0, 2, n), tuple(int(v) for v in rng.integers(0, 6, 2)))


def rings_in_a_row(sizes, seed, spread=4000, **kw):
    """one run: rings of the given vertex counts at seeded places"""
    rng = np.random.default_rng(seed)
    return pack([ring(int(rng.integers(0, spread)) + 2 * radius(m), int(rng.integers(0, spread)) + 2 * radius(m), radius(m), m, float(rng.uniform(0, 6))) for m in sizes], **kw)


def equidistant():
    """one square around the cursor's column, stored from a far vertex: vertices 1 and 2 are equally near (20 steps), 0 and 3 are 40 away"""
    q = np.roll(square(10, 20, 20)[:-1], 1, 0)
    return pack([np.concatenate([q, q[:1]])], start=(20, 0))


def all_open(seed=3, n=40):
    rng = np.random.default_rng(seed)
    return pack([rng.integers(0, 500, (int(rng.integers(2, 6)), 2)) for _ in range(n)], rng.permutation(n), rng.integers(0, 2, n))


def mixed_small(seed=4):
    """A, B, A and 2-point strokes among rings"""
    return pack([square(0, 0, 10), np.array([[30, 5], [40, 5], [30, 5]]), square(50, 0, 10), line(70, 70, 80, 80), ring(100, 100, 9, 7), np.array([[5, 5], [6, 6], [5, 5]]),
                 ring(20, 80, 12, 5)], start=(60, 60))


def placements():
    """name -> case: where the runs lie in the sequence"""
    r = lambda i, m=6: ring(100 + 90 * i, 100 + 37 * (i % 3), 20, m, 0.3 * i)
    o = lambda i: line(60 + 80 * i, 300, 90 + 80 * i, 260)
    return {
        "ring_first": pack([r(0), o(1), o(2)]),
        "ring_last": pack([o(0), o(1), r(2)]),
        "run_between_open": pack([o(0), r(1), r(2), r(3), o(4)]),
        "two_runs": pack([r(0), r(1), o(2), r(3), r(4), r(5), o(6)]),
        "one_run": pack([r(i) for i in range(6)], start=(500, 500)),
    }


def lattice(seed=5, n=30):
    """axis-parallel squares on a lattice of pitch 10: most candidates tie"""
    rng = np.random.default_rng(seed)
    return pack([square(10 * int(x), 10 * int(y), 10) for x, y in rng.integers(0, 6, (n, 2))], rng.permutation(n), rng.integers(0, 2, n), (25, 25))


def figure_eight():
    """a ring that passes (20, 20) twice: two candidates on one grid point; the cursor stands on it"""
    eight = np.array([[20, 20], [30, 10], [40, 20], [30, 30], [20, 20], [10, 30], [0, 20], [10, 10], [20, 20]])
    return pack([line(0, 0, 20, 20), eight, square(60, 20, 10), eight[::-1] + 100], rev=[0, 1, 0, 0])


EDGE_SIZES = (3, 63, 64, 65, 257)


def wave_edges(seed=6):
    """neighbouring rings of 3, 63, 64, 65 and 257 vertices, every ordered pair adjacent somewhere in the one run"""
    sizes = []
    for a in EDGE_SIZES:
        for b in EDGE_SIZES:
            sizes += [a, b]
    return rings_in_a_row(sizes, seed)


def chunk_edges(seed=14):
    """rings on both sides of the 512 vertices one block takes at a time, small ones between them: the walk changes between its two forms and back"""
    return rings_in_a_row([40, 511, 512, 513, 512, 100, 600, 257, 3, 513, 513, 64, 512, 256, 1025, 9], seed, spread=6000, start=(3000, 0))


def around_hand_over(other, seed=7):
    """a run 64, 1024, `other`, 64: the middle layer has 1024 * other pairs, with short layers on both sides of it"""
    return rings_in_a_row([64, 1024, other, 64], seed, spread=9000, start=(0, 9000))


def one_by_3000(seed=8):
    """a point in front of a ring of 3000 and a ring of 3000 in front of a point; a triangle on either side of a ring of 3000"""
    rng = np.random.default_rng(seed)
    big = lambda: ring(int(rng.integers(4000, 9000)), int(rng.integers(4000, 9000)), 3000, 3000, float(rng.uniform(0, 6)))
    tri = lambda: ring(int(rng.integers(100, 9000)), int(rng.integers(100, 9000)), 50, 3)
    return pack([line(5, 5, 100, 7000), big(), line(9000, 100, 9100, 90), tri(), big(), tri(), line(1, 1, 2, 2)])


def pair_3000(seed=9):
    return rings_in_a_row([3000, 3000], seed, spread=9000, start=(12000, 0))


def triangles(n=2000, seed=10):
    rng = np.random.default_rng(seed)
    c = rng.integers(20, 5000, (n, 2))
    return pack([ring(int(x), int(y), 15, 3, float(t)) for (x, y), t in zip(c, rng.uniform(0, 6, n))])


def corners(n=12, seed=11):
    """coordinates 0 and 2^30 only: squares the size of the whole range, every third stroke a diagonal of it"""
    rng = np.random.default_rng(seed)
    sq = np.array([[0, 0], [TOP, 0], [TOP, TOP], [0, TOP]])
    strokes = []
    for i in range(n):
        if i % 3 == 2:
            a = rng.integers(0, 2, 2) * TOP
            strokes.append(np.array([a, TOP - a]))
        else:
            q = np.roll(sq, int(rng.integers(0, 4)), 0)
            strokes.append(np.concatenate([q, q[:1]]))
    return pack(strokes, start=(TOP, 0))


def far_apart(n=10):
    """squares in two opposite corners of the range in turn, coordinates 0 and 2^30 among them: every approach is 2^30 - 80 steps at least, and the
    cost-to-go of the first ring leaves 32 bits"""
    strokes = [np.roll(square(0, 0, 40)[:-1], i, 0) if i % 2 else np.roll(square(TOP - 40, TOP - 40, 40)[:-1], i, 0) for i in range(n)]
    return pack([np.concatenate([q, q[:1]]) for q in strokes], start=(0, TOP))


def shuffled(seed=12, n=40):
    """a non-identity order with rev set on open and closed strokes"""
    rng = np.random.default_rng(seed)
    strokes = [ring(int(x), int(y), 25, int(m), float(t)) if m else rng.integers(0, 900, (3, 2)) + 1
               for (x, y), m, t in zip(rng.integers(50, 900, (n, 2)), rng.choice([0, 5, 9, 16], n), rng.uniform(0, 6, n))]
    return pack(strokes, rng.permutation(n), rng.integers(0, 2, n), (450, 0))


def random_rings(n=3000, seed=13, size=20000):
    """n rings of 16 - 48 vertices at seeded places: (off, pts)"""
    rng = np.random.default_rng(seed)
    c = rng.integers(100, size, (n, 2)); m = rng.integers(16, 49, n); t = rng.uniform(0, 6, n)
    off, pts, _, _, _ = pack([ring(int(c[i, 0]), int(c[i, 1]), 60, int(m[i]), float(t[i])) for i in range(n)])
    return off, pts


def tool_gcode(rows=5, cols=6):
    """a G-code text in mm: a grid of circles of 12 chords and squares, with an open stroke after every third shape"""
    out = ["G21 G90 M5"]
    for i in range(rows * cols):
        cx, cy = 20.0 + 30.0 * (i % cols), 20.0 + 40.0 * (i // cols)
        if i % 2:
            p = [(cx - 8, cy - 8), (cx + 8, cy - 8), (cx + 8, cy + 8), (cx - 8, cy + 8), (cx - 8, cy - 8)]
        else:
            p = [(cx + 9 * np.cos(2 * np.pi * j / 12 + i), cy + 9 * np.sin(2 * np.pi * j / 12 + i)) for j in range(12)]
            p.append(p[0])
        if i % 3 == 2:
            p = p + [(cx, cy)]                          # a tail: no longer closed
        out += ["G0 X%.3f Y%.3f" % p[0], "M3"] + ["G1 X%.3f Y%.3f" % q for q in p[1:]] + ["M5"]
    return "\n".join(out) + "\n"


def tool_svg(rows=3, cols=4):
    """a drawing of circles, rectangles and closed paths in two stroke colours, with a few open lines among them"""
    out = ['<svg xmlns="http://www.w3.org/2000/svg" width="200" height="160" viewBox="0 0 200 160">']
    for i in range(rows * cols):
        cx, cy = 25 + 50 * (i % cols), 25 + 50 * (i // cols)
        col = "#f00" if i % 2 else "#00f"
        if i % 3 == 0:
            out.append(f'<circle cx="{cx}" cy="{cy}" r="18" fill="none" stroke="{col}"/>')
        elif i % 3 == 1:
            out.append(f'<rect x="{cx - 15}" y="{cy - 12}" width="30" height="24" fill="none" stroke="{col}"/>')
        else:
            out.append(f'<path fill="none" stroke="{col}" d="M{cx - 16} {cy + 14} L{cx} {cy - 16} L{cx + 16} {cy + 14} Z"/>')
            out.append(f'<line stroke="{col}" x1="{cx - 5}" y1="{cy}" x2="{cx + 5}" y2="{cy + 6}"/>')
    return ("\n".join(out) + "\n</svg>\n").encode()


TOOL_SVG = tool_svg()
TOOL_SVG_ARGS = ["--pen-colors", "rgbk", "--allow-reverse"]
