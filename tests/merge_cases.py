"""TEST INFRASTRUCTURE: the inputs of the --merge-paths tests (tests/test_merge_host.py on the double, tests/test_gpu_merge.py on the device): the smallest
shapes that can break the rule or the kernel, the drawing of the whole-tool tests as G-code and as SVG, and a reader of the strokes of a stream."""
import numpy as np

TOP = 1 << 30


def paths(lists, groups=None, n_groups=1):
    """[[(x, y), ...], ...] -> (off, pts, group, n_groups)"""
    off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
    pts = np.asarray([q for p in lists for q in p], np.int32).reshape(-1, 2)
    return off, pts, np.zeros(len(lists), np.int32) if groups is None else np.asarray(groups, np.int32), n_groups


def chain(k, closed, seed, long_member=None, flips=True):
    """a polyline through k + 1 distinct points (closed: through k, back to the first) exploded into k two-point members, file order shuffled, about half
    of them flipped (none without `flips`: the chain then joins without REVERSE too); long_member = (index, points): that member gets so many points
    instead of two, and is flipped"""
    rng = np.random.default_rng(seed)
    P = np.stack([np.arange(k + 1) * 3 + 7, (np.arange(k + 1) * 37) % 101 + rng.integers(0, 2, k + 1) * 200], 1)      # distinct x: no two points coincide
    if closed:
        P[k] = P[0]
    members = [[P[i], P[i + 1]] for i in range(k)]
    if long_member is not None:
        i, m = long_member
        zig = [(int(P[i][0]), 1000 + j) if j % 2 else (int(P[i][0]) + 1, 1000 + j) for j in range(m - 2)]              # off every node, no two neighbours equal
        members[i] = [P[i]] + zig + [P[i + 1]]
    flip = (rng.random(k) < 0.5) & flips
    if long_member is not None:
        flip[long_member[0]] = True
    members = [m[::-1] if f else m for m, f in zip(members, flip)]
    return paths([[tuple(int(v) for v in q) for q in members[i]] for i in rng.permutation(k)])


def cycle_lowest_in_the_middle(k):
    """a k-cycle whose lowest member is neither the first nor the last path of the file: a lone path stands in front of the ring and one behind it, and the
    ring's members are listed out of their order round the ring (ring member 1 first, member 0 last)"""
    P = [(10 * i + 5, (i * i) % 7 + 3) for i in range(k)]
    ring = [[P[i], P[(i + 1) % k]] for i in range(k)]
    return paths([[(900, 900), (901, 950)]] + [ring[(i + 1) % k] for i in range(k)] + [[(800, 800), (801, 850)]])


def random_grid(n=4000, side=40, n_groups=3, closed=0.3, seed=3):
    """ends on a side x side grid (every degree occurs), 30 % of the paths closed, 2 .. 5 points each, interior points off the grid and no two neighbours equal"""
    rng = np.random.default_rng(seed)
    lists = []
    for p in range(n):
        a = tuple(rng.integers(0, side, 2).tolist())
        cl = rng.random() < closed
        b = a
        while not cl and b == a:
            b = tuple(rng.integers(0, side, 2).tolist())
        inner = [(100 + j, int(rng.integers(0, 50))) for j in range(int(rng.integers(1 if cl else 0, 4)))]
        lists.append([a] + inner + [b])
    return paths(lists, rng.integers(0, n_groups, n), n_groups)


def small_cases():
    """name -> (off, pts, group, n_groups)"""
    A, B, C, D = (5, 5), (9, 1), (9, 9), (2, 8)
    c = {
        "one_open": paths([[A, B]]),
        "one_closed": paths([[A, B, C, A]]),                                    # degree 2 from one path: no join
        "tail_head": paths([[A, B], [B, C]]),
        "tail_tail": paths([[A, B], [C, B]]),                                   # joined only with REVERSE
        "head_head": paths([[B, A], [B, C]]),
        "three_on_a_node": paths([[A, B], [B, C], [B, D], [C, (20, 20)], [(30, 30), D]]),      # nothing at B; the far ends of paths 1 and 2 still join
        "closed_plus_end": paths([[A, B, C, A], [D, A]]),
        "two_cycle": cycle_lowest_in_the_middle(2),
        "two_cycle_reverse_only": paths([[(50, 50), (60, 60)], [B, C, D], [B, (7, 7), D], [(70, 70), (80, 80)]]),      # head to head and tail to tail
        "three_cycle": cycle_lowest_in_the_middle(3),
        "five_cycle": cycle_lowest_in_the_middle(5),
        "duplicate": paths([[A, B, C], [A, B, C]]),                             # a cycle only with REVERSE
        "two_groups": paths([[A, B], [B, C]], [0, 1], 2),                       # the same point in two groups: no join
        "x_only": paths([[A, (9, 1)], [(10, 1), C]]),
        "y_only": paths([[A, (9, 1)], [(9, 2), C]]),
        "swapped": paths([[A, (9, 1)], [(1, 9), C]]),
        "group_only": paths([[A, B], [B, C], [C, D]], [2, 2, 63], 64),
        "corners": paths([[(0, 0), (TOP, 0)], [(TOP, 0), (TOP, TOP)], [(TOP, TOP), (0, TOP)], [(0, TOP), (0, 0)], [(0, TOP), (TOP, 0)]]),
        "long_member": chain(12, False, 41, long_member=(5, 5000)),
    }
    for k in (63, 64, 65, 255, 256, 257, 1025):
        c[f"chain_{k}"] = chain(k, False, k)
        c[f"cycle_{k}"] = chain(k, True, 1000 + k)
        c[f"cycle_{k}_forwards"] = chain(k, True, 2000 + k, flips=False)
    return c


# ------------------------------------------------------------------ the drawing of the whole-tool tests
def _drawing():
    """strokes in mm, each a list of points: a square as four strokes, a diagonal that meets two of its corners (three ends there), a triangle as three
    strokes, and a 300-point sine exploded into two-point strokes in a scattered file order"""
    sq = [(10, 10), (60, 10), (60, 60), (10, 60)]
    strokes = [[sq[i], sq[(i + 1) % 4]] for i in range(4)] + [[sq[0], sq[2]]]
    tri = [(100, 20), (120, 20), (110, 40)]
    strokes += [[tri[i], tri[(i + 1) % 3]] for i in (1, 2, 0)]
    sine = [(20 + 0.25 * i, round(120 + 30 * float(np.sin(i / 20.0)), 3)) for i in range(300)]
    strokes += [[sine[i], sine[i + 1]] for i in ((7 * j) % 299 for j in range(299))]
    return strokes, 5 + 3                                      # how many strokes are not the sine's


def tool_gcode():
    strokes, _ = _drawing()
    out = ["G21", "G90", "M5"]
    for s in strokes:
        out += ["G0 X%g Y%g" % s[0], "M3"] + ["G1 X%g Y%g" % q for q in s[1:]] + ["M5"]
    return "\n".join(out) + "\n"


def tool_svg():
    """the same strokes as <line> elements in two stroke colours: the shapes red, the sine blue"""
    strokes, shapes = _drawing()
    body = "".join('<line x1="%g" y1="%g" x2="%g" y2="%g" stroke="%s"/>' % (*s[0], *s[1], "#f00" if i < shapes else "#00f") for i, s in enumerate(strokes))
    return ('<svg xmlns="http://www.w3.org/2000/svg" width="200" height="200" viewBox="0 0 200 200">' + body + "</svg>").encode()


TOOL_SVG_ARGS = ["--merge-paths", "--pen-colors", "#f00,#00f"]


# ------------------------------------------------------------------ what a stream draws
def strokes_of(data):
    """the pen-down strokes of a stream, in order: [(colour, [(x, y) of the pen-down position and after every step])]"""
    import stream_preview_double as SPD
    _, kind, val = SPD.decode(data)
    x = y = 0
    col, down, out = 0, False, []
    for k, v in zip(kind.tolist(), val.tolist()):
        if k == SPD.K_STEP:
            x += int(SPD.DX[v]); y += int(SPD.DY[v])
            if down:
                out[-1][1].append((x, y))
        elif k == SPD.K_COLOR:
            col = v
        elif k == SPD.K_PEN:
            if v == 2 and not down:
                out.append((col, [(x, y)]))
            down = v == 2
    return out
