"""TEST INFRASTRUCTURE: the named drawings of --hatch-connect (include/orip.h: orip_gcode_hatch_link), shapes in steps.  Unless a case says otherwise:
spacing 40, inset 27, serpentine, horizontal, reach 80, the lines those of hatch_double.hatch_direction.  A case is a dict of the seven arguments of
hatch_link_double.hatch_link / Device.gcode_hatch_link: off, pts, cls, ring_off, ring_pts, ring_group, reach."""
import numpy as np

import hatch_double as HD

TOP = 1 << 30
SQUARE = [(100, 100), (1100, 100), (1100, 1100), (100, 1100)]
L_SHAPE = [(x + 100, y + 100) for x, y in [(0, 0), (1200, 0), (1200, 400), (400, 400), (400, 1200), (0, 1200)]]
U_SHAPE = [(x + 100, y + 100) for x, y in [(0, 0), (1200, 0), (1200, 1200), (800, 1200), (800, 400), (400, 400), (400, 1200), (0, 1200)]]
SLIT = [(100, 100), (1100, 100), (1100, 900), (610, 900), (610, 300), (590, 300), (590, 900), (100, 900)]


def ngon(cx, cy, r, k):
    a = np.arange(k) * (2 * np.pi / k)
    return [(int(x), int(y)) for x, y in np.stack([np.rint(cx + r * np.cos(a)), np.rint(cy + r * np.sin(a))], 1).tolist()]


def case(strokes, cls, rings, ring_group, reach=80):
    """strokes and rings as lists of point lists"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in strokes])]).astype(np.int64)
    pts = np.asarray([q for s in strokes for q in s], np.int32).reshape(-1, 2)
    r_off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    r_pts = np.asarray([q for r in rings for q in r], np.int32).reshape(-1, 2)
    return dict(off=off, pts=pts, cls=np.asarray(cls, np.int32).reshape(-1), ring_off=r_off, ring_pts=r_pts, ring_group=np.asarray(ring_group, np.int32).reshape(-1), reach=int(reach))


def hatched(shapes, spacing=40, inset=27, serpentine=True, directions=(False,), reach=80, group_ids=None):
    """shapes: a list of shapes, each a list of rings; hatched as the tool hatches (every direction over all shapes, the shapes ascending) -> case"""
    rings = [r for sh in shapes for r in sh]
    gid = [g for g, sh in enumerate(shapes) for _ in sh]
    ids = list(range(len(shapes))) if group_ids is None else list(group_ids)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rings])])
    q = np.asarray([p for r in rings for p in r], np.int64)
    strokes, cls = [], []
    for vert in directions:
        for g in range(len(shapes)):
            seg, _, _ = HD.hatch_direction(off, q, [g if v == g else -1 for v in gid], spacing, inset, serpentine, vert)
            strokes += [[(int(s[0]), int(s[1])), (int(s[2]), int(s[3]))] for s in seg]
            cls += [2 * ids[g] + int(vert)] * len(seg)
    return case(strokes, cls, rings, [ids[g] for g in gid], reach)


def hand_lists():
    """hand-built lists: the rule's small print.  One square ring (0, 0)-(1000, 1000) as shape 0 unless the case brings its own"""
    box = [[(0, 0), (1000, 0), (1000, 1000), (0, 1000)]]
    H = {}
    # one END (line 0), two STARTs at equal distance, above and below: the lower index wins; and one START (line 2) with two ENDs at equal distance
    H["tie_from_one_end"] = case([[(100, 500), (500, 500)], [(500, 540), (100, 540)], [(500, 460), (100, 460)]], [0, 0, 0], box, [0])
    H["tie_from_one_start"] = case([[(100, 540), (500, 540)], [(100, 460), (500, 460)], [(500, 500), (100, 500)]], [0, 0, 0], box, [0])
    # a's best is b (30 away), b's best is a2 (10 away): a stays single, a2 -> b
    H["not_mutual"] = case([[(100, 500), (500, 500)], [(100, 540), (500, 520)], [(500, 530), (100, 530)]], [0, 0, 0], box, [0])
    H["coincident"] = case([[(100, 500), (500, 500)], [(500, 500), (500, 700)], [(500, 730), (100, 730)]], [0, 0, 0], box, [0])
    H["class_of_one_line"] = case([[(100, 500), (500, 500)], [(500, 540), (100, 540)], [(100, 580), (500, 580)]], [0, 2, 0], box + [[(0, 0), (900, 0), (900, 900)]], [0, 1])
    H["three_points_take_no_part"] = case([[(100, 500), (500, 500)], [(500, 540), (300, 550), (100, 540)], [(500, 560), (100, 560)]], [0, 0, 0], box, [0])
    H["no_class"] = case([[(100, 500), (500, 500)], [(500, 540), (100, 540)]], [-1, -1], box, [0])
    H["no_rings"] = case([[(100, 500), (500, 500)], [(500, 540), (100, 540)]], [0, 0], [], [])
    H["shape_without_rings"] = case([[(100, 500), (500, 500)], [(500, 540), (100, 540)]], [4, 4], box, [0])
    H["mixed_with_outlines"] = case([box[0] + box[0][:1], [(100, 500), (500, 500)], [(7, 7), (9, 9), (7, 9)], [(500, 540), (100, 540)], [(100, 580), (500, 580)]], [-1, 0, -1, 0, 0],
                                    box, [0])
    return H


def many_starts():
    """70 STARTs on one grid point within reach of one END: more candidates than a wave has lanes; the lowest one is linked"""
    box = [[(0, 0), (1000, 0), (1000, 1000), (0, 1000)]]
    return case([[(100, 500), (500, 500)]] + [[(500, 540), (100 + k, 540 + k)] for k in range(70)], [0] * 71, box, [0])


def far_corner():
    """coordinates at 2^30 - 1 with ring points at -2^30: orientation products whose terms reach 2^62.  Three shapes for the same three lines, whose links
    run up x = t - 100 (from y = t - 60) and up x = t - 500 (from y = t - 20): the whole plane's square (both link); the half plane y > x + 60 (the first
    link starts outside it); the half plane y > x + 40, on whose edge the first link's start lies exactly (a product of 2^62 less one of 2^62 is 0)"""
    t = TOP - 1
    strokes = [[(t - 500, t - 60), (t - 100, t - 60)], [(t - 100, t - 20), (t - 500, t - 20)], [(t - 500, t), (t - 100, t)]]
    square = [(-TOP, -TOP), (TOP, -TOP), (TOP, TOP), (-TOP, TOP)]
    return [case(strokes, [0, 0, 0], [ring], [0]) for ring in (square, [(-TOP, -TOP + 60), (TOP - 60, TOP), (-TOP, TOP)], [(-TOP, -TOP + 40), (TOP - 40, TOP), (-TOP, TOP)])]


def random_lines(seed=11, n=200, rings=5):
    """200 short 2-point lines with random classes over 5 random rings on a small grid: ties, touching and collinear links are the rule"""
    rng = np.random.default_rng(seed)
    groups = np.sort(rng.integers(0, 3, rings))
    rr = [HD.star(rng, 60, 60, 55, 7).tolist() for _ in range(rings)]
    strokes, cls = [], []
    while len(strokes) < n:
        a = rng.integers(10, 110, 2); b = a + rng.integers(-12, 13, 2)
        if (a != b).any() and (b >= 0).all():
            strokes.append([tuple(a.tolist()), tuple(b.tolist())]); cls.append(int(rng.integers(-1, 6)))
    return case(strokes, cls, [[tuple(p) for p in r] for r in rr], groups, reach=10)


def cases():
    C = {}
    C["square"] = hatched([[SQUARE]])
    C["l_shape"] = hatched([[L_SHAPE]])
    C["u_shape"] = hatched([[U_SHAPE]])
    C["slit"] = hatched([[SLIT]], inset=5)
    C["circle_64"] = hatched([[ngon(1000, 1000, 1000, 64)]])
    C["ring_with_hole"] = hatched([[ngon(1000, 1000, 1000, 48), ngon(1000, 1000, 400, 24)]])
    C["cross_hatch"] = hatched([[SQUARE]], directions=(False, True))
    C["two_squares"] = hatched([[SQUARE], [[(x + 1030, y) for x, y in SQUARE]]], inset=10)         # 30 apart: the ends across the gap lie 50 apart, within reach
    C["inset_0"] = hatched([[SQUARE]], inset=0)
    C["reach_39"] = hatched([[SQUARE]], reach=39)
    C["reach_40"] = hatched([[SQUARE]], reach=40)
    C["no_serpentine"] = hatched([[SQUARE]], serpentine=False)
    C["polygon_of_70_edges"] = hatched([[ngon(600, 600, 500, 70)]])
    C["polygon_of_3000_edges"] = hatched([[ngon(600, 600, 500, 3000)]])
    C["sparse_group_ids"] = hatched([[SQUARE], [[(x + 2000, y) for x, y in L_SHAPE]]], group_ids=(3, 900000000))
    rng = np.random.default_rng(7)
    for k in range(3):
        C[f"star_{k}"] = hatched([[[tuple(p) for p in HD.star(rng, 1100, 1100, 1000, 9).tolist()]]])
    shapes = [[[tuple(p) for p in HD.star(rng, 700 + 1500 * (k % 4), 700 + 1500 * (k // 4), 650, 9).tolist()]] for k in range(15)] + [[[(x + 4600, y + 4600) for x, y in SQUARE]]]
    C["sixteen_shapes"] = hatched(shapes, directions=(False, True))                                 # 900 lines or so: several blocks, two families, shapes side by side
    C["random_lines"] = random_lines()
    C["many_starts"] = many_starts()
    C["far_corner_open"], C["far_corner_outside"], C["far_corner_on_edge"] = far_corner()
    C.update(hand_lists())
    C["empty"] = case([], [], [SQUARE], [0])
    return C


def args(c):
    return c["off"], c["pts"], c["cls"], c["ring_off"], c["ring_pts"], c["ring_group"], c["reach"]


# ------------------------------------------------------------------ the consequences the rule states, which need no double
def check_consequences(c, out):
    """every stated consequence of include/orip.h on a result (off, pts, member_off, member, stats) of case c, with this file's own arithmetic"""
    import hatch_link_double as LD
    off, pts, moff, member, st = out
    i_off, i_pts, cls = c["off"].tolist(), [tuple(q) for q in c["pts"].tolist()], c["cls"].tolist()
    n = len(i_off) - 1
    o_pts = [tuple(q) for q in np.asarray(pts).tolist()]
    assert st["paths_out"] == len(off) - 1 == n - st["links"] and st["points_out"] == len(o_pts) == len(i_pts) - st["coincident"]
    assert len(moff) == len(off) and moff[0] == 0 and moff[-1] == n and sorted(np.asarray(member).tolist()) == list(range(n))
    shapes = LD.shape_edges(c["ring_off"].tolist(), [tuple(q) for q in c["ring_pts"].tolist()], c["ring_group"].tolist())
    firsts, links, steps, coin = [], 0, 0, 0
    for k in range(len(off) - 1):
        mem = np.asarray(member[moff[k]:moff[k + 1]]).tolist()
        firsts.append(mem[0])
        want = []
        for a, b in zip([None] + mem[:-1], mem):
            s = i_pts[i_off[b]:i_off[b + 1]]
            if a is not None:                                            # a link END a -> START b
                e = i_pts[i_off[a] + 1]
                assert a < b and cls[a] == cls[b] >= 0 and i_off[a + 1] - i_off[a] == 2 and len(s) == 2
                dx, dy = s[0][0] - e[0], s[0][1] - e[1]
                assert dx * dx + dy * dy <= c["reach"] ** 2
                edges = shapes.get(cls[a] >> 1, [])
                assert LD.inside(e, edges) and not any(LD.segments_meet(e, s[0], p, q) for p, q in edges)
                links += 1; steps += max(abs(dx), abs(dy)); coin += e == s[0]
                if e == s[0]:
                    s = s[1:]
            want += s
        assert o_pts[off[k]:off[k + 1]] == want                          # every output segment is an input segment or a link, in order
    assert firsts == sorted(firsts) and (links, steps, coin) == (st["links"], st["link_steps"], st["coincident"])
    assert st["lines"] == sum(1 for k in range(n) if cls[k] >= 0 and i_off[k + 1] - i_off[k] == 2) and st["links"] <= st["eligible"] <= st["in_reach"]


# ------------------------------------------------------------------ the whole tool
# an L, hatched into one zigzag; a rectangle of another colour beside it; and a rectangle painted over the L's leg, which cuts the zigzag under --occlude
TOOL_SVG_L = b"""<svg xmlns="http://www.w3.org/2000/svg" width="200" height="200" viewBox="0 0 200 200">
 <path d="M10 10 H130 V50 H50 V130 H10 Z" fill="#88f" stroke="#00f"/>
</svg>
"""
TOOL_SVG = b"""<svg xmlns="http://www.w3.org/2000/svg" width="200" height="200" viewBox="0 0 200 200">
 <path d="M10 10 H130 V50 H50 V130 H10 Z" fill="#88f" stroke="#00f"/>
 <rect x="140" y="20" width="50" height="60" fill="#f88" stroke="#f00"/>
 <rect x="30" y="70" width="60" height="40" fill="#88f" stroke="#00f"/>
</svg>
"""
TOOL_ARGS = ["--scale", "1", "--margin-mm", "0", "--steps-per-mm", "10", "--hatch-spacing-mm", "4"]


class HatchLinkDouble:
    """hatch_link_fn of orip.svg.build_stream_from_svg through the doubles: the rings converted by occlude_double.rings_to_steps, the pass by hatch_link_double"""
    def __init__(self): self.calls = 0; self.out = None; self.rings = None; self.cls = None; self.inp = None; self.reach = None

    def __call__(self, paths, off, pts, cls, ring_sub, ring_group, m, clamp, reach):
        import hatch_link_double as LD
        import occlude_double as OD
        r_off, r_pts = OD.rings_to_steps(np.asarray(paths[0]), np.asarray(paths[1]), np.asarray(ring_sub).tolist(), m, clamp)
        self.rings = (r_off, r_pts, np.asarray(ring_group), clamp); self.cls = np.asarray(cls); self.inp = (np.asarray(off), np.asarray(pts)); self.reach = reach
        self.out = LD.hatch_link(off, pts, cls, r_off, r_pts, ring_group, reach)
        self.calls += 1
        return self.out
