"""No GPU: every case of cross_cases.py reaches what its name says.  The oracle's parts (O.cut_poly, O.tiny_and_taps10, O.min_enclosing_circle, O.stage10_layer)
give the pieces, the circles and the rasters; the branch conditions of csrc/vector10.hip are re-evaluated in numpy on them (cross_cases.step_points, slot_counts,
branch_of, fate_of, mec_trace) and asserted case by case: a case that stops reaching its branch fails here.  The small cases also carry answers worked out by hand,
so that the oracle is not their only witness, and O.min_enclosing_circle is held bit for bit against tests/golden/cv2_standin.py on every point set of the tap
cases."""
import sys

import numpy as np
import pytest

from oracle import oracle as O
import cross_cases as X
from util import same_polys, GOLDEN

sys.path.insert(0, GOLDEN)
import cv2_standin  # noqa: E402


def tl(polys):
    return [[tuple(int(v) for v in q) for q in np.asarray(p).reshape(-1, 2)] for p in polys]


def cut_with(poly, forb, lookup):
    """the cut with another rule for the pixel a step point reads (the emitted point stays truncated); pieces in cut order"""
    H, W = forb.shape; out = []; cur = []
    for qx, qy in X.step_points(poly):
        xi, yi = int(lookup(float(qx))), int(lookup(float(qy)))
        if 0 <= xi < W and 0 <= yi < H and forb[yi, xi]:
            if len(cur) >= 2: out.append(cur)
            cur = []
        else:
            cur.append((int(qx), int(qy)))
    if len(cur) >= 2: out.append(cur)
    return out


HALF_EVEN, HALF_UP, TRUNC = np.rint, lambda v: np.floor(v + 0.5), np.trunc


def cut_layer(c, lookup):
    (_, forb) = X.raster_after(O, c, len(c["layers"]) - 1)
    return [p for poly in c["layers"][-1][0] for p in cut_with(poly, forb, lookup)], forb


def oracle_cut(c, forb):
    return tl([p for poly in c["layers"][-1][0] for p in O.cut_poly(poly, forb)])


# ---------------------------------------------------------------- A. cut
@pytest.mark.parametrize("name", sorted(X.CUT))
def test_step_points_restate_the_cut(name):
    """cross_cases.step_points with the half-even lookup IS the oracle's cut, on every cut case (so what the tests below read off the step points holds)"""
    c = X.CUT[name]
    mine, forb = cut_layer(c, HALF_EVEN)
    assert mine == oracle_cut(c, forb)
    assert forb.any()


def test_rounding_triple_tells_the_three_rules_apart():
    c = X.CUT["rounding_triple"]
    he, forb = cut_layer(c, HALF_EVEN)
    assert tl(X.raster_after(O, c, 1)[0][0][0]) == [[(11, 11), (12, 11)]] and int((forb != 0).sum()) == 2
    q = X.step_points(c["layers"][1][0][0])
    assert [tuple(v) for v in q[1::2].tolist()] == [(10.5, 10.5), (11.5, 11.5), (12.5, 12.5), (13.5, 13.5)]
    hu, _ = cut_layer(c, HALF_UP); tr, _ = cut_layer(c, TRUNC)
    assert hu == X.TRIPLE_HALF_UP and tr == X.TRIPLE_TRUNC
    assert sorted(he) == sorted(X.CUT_LITERAL["rounding_triple"]) and he != hu and he != tr and hu != tr
    assert tl(X.want(O, c)[1][0]) == X.CUT_LITERAL["rounding_triple"]


def test_ends_and_short_runs():
    c = X.CUT["ends_and_short_runs"]
    _, forb = cut_layer(c, HALF_EVEN)
    free = [not forb[20, x] for x in range(10, 31)]
    runs = [len(r) for r in "".join("1" if f else "0" for f in free).split("0") if r]
    assert not free[0] and not free[-1] and runs == [2, 1, 14]
    assert tl(X.want(O, c)[1][0]) == X.CUT_LITERAL["ends_and_short_runs"]


def test_across_zero_and_beyond_the_far_edges():
    """step points whose pixel lies outside the canvas (never forbidden) while the emitted, truncated point lies inside -- on all four sides; reading the raster at the
    truncated point instead changes the answer"""
    for name, lo in (("across_zero", True), ("beyond_far_edges", False)):
        c = X.CUT[name]
        q = np.concatenate([X.step_points(p) for p in c["layers"][-1][0]]).astype(np.float64)
        for axis, size in ((0, c["W"]), (1, c["H"])):
            v = q[:, axis]
            hit = (np.rint(v) == -1) & (np.trunc(v) == 0) if lo else (np.rint(v) == size) & (np.trunc(v) == size - 1)
            assert hit.any(), (name, axis)
        assert (q != np.rint(q)).any()
        he, forb = cut_layer(c, HALF_EVEN); tr, _ = cut_layer(c, TRUNC)
        assert he != tr and len(he) > len(c["layers"][-1][0])          # something is cut, and the rule matters
    q = np.concatenate([X.step_points(p) for p in X.CUT["across_zero"]["layers"][-1][0]])
    assert ((q > -1) & (q < 0)).any(axis=0).all()          # truncation toward zero, not floor, on both axes


def test_repeated_vertices_and_one_point_polylines():
    c = X.CUT["repeated_vertices"]
    cnt = [X.slot_counts(p) for p in c["layers"][1][0]]
    assert cnt[0][:2] == [1, 0] and cnt[1][2:4] == [0, 0] and cnt[2][-1] == 0 and cnt[3] == [1, 0, 0, 0] and cnt[4] == [1, 0, 0, 1, 0]
    empty = np.zeros((30, 40), np.uint8)
    assert O.cut_poly(c["layers"][1][0][3], empty) == []          # one point repeated: one slot, a run of one
    got = X.want(O, c)[1][0]
    assert sorted(len(p) for p in got) == [2, 3, 5, 6]          # the third polyline is cut at x = 8 and its end, (9, 12), stays alone; the fourth gives nothing
    c = X.CUT["one_point_polylines"]
    for l, idx in ((0, (0, 2)), (1, (0, 2, 3, 5)), (2, (0, 1))):
        assert [i for i, p in enumerate(c["layers"][l][0]) if len(p) == 1] == list(idx)
    w = X.want(O, c)
    assert tl(w[0][0]) == [[(6, 6), (7, 6)]] and w[2] == ([], [])
    assert sorted(sorted(p) for p in tl(w[1][0])) == [[(2, 6), (3, 6), (4, 6), (5, 6)], [(2, 8), (3, 8), (4, 8), (5, 8), (6, 8), (7, 8), (8, 8), (9, 8)], [(8, 6), (9, 6)]]


def test_long_polylines_pass_the_block_stride():
    c = X.CUT["long_polylines"]
    assert [len(p) for p in c["layers"][1][0]] == [256, 257, 600]
    assert all(X.slot_counts(p) == [1] * len(p) for p in c["layers"][1][0])
    he, forb = cut_layer(c, HALF_EVEN)
    for p in c["layers"][1][0]:
        v = p.reshape(-1, 2); blocked = [i for i in range(len(v)) if forb[v[i, 1], v[i, 0]]]
        assert blocked == [i for i in (255, 256, 511, 512) if i < len(v)], len(v)
    assert sorted(len(p) for p in he) == [87, 254, 255, 255, 255]          # 256: the last vertex is forbidden; 257: the last two; 600: 255 | 254 | 87


def test_long_oblique_has_float32_products_to_round():
    c = X.CUT["long_oblique"]
    for p in c["layers"][1][0]:
        q = X.step_points(p); v = p.reshape(-1, 2).astype(np.float64)
        assert len(q) > 38000
        t = (np.arange(1, len(q)) / float(len(q) - 1))
        exact = v[0] + (v[1] - v[0]) * t[:, None]
        assert (np.trunc(exact) != np.trunc(q[1:].astype(np.float64))).any()          # the float32 evaluation decides some of the emitted points
    he, forb = cut_layer(c, HALF_EVEN)
    assert len(he) >= 4 and max(len(p) for p in he) > 10000


@pytest.fixture(scope="module")
def large():
    c = X.large_case()
    return c, X.want(O, c)[0]


def test_large_layer(large):
    c, (lines, taps) = large
    polys = c["layers"][0][0]
    assert len(polys) == X.LARGE_N > 65535                                 # the grid stride of k_cut_counts
    p = X.prm_of(c)
    seen = set()
    for k in (0, 1, 2299, 2300, 65535, 65536, X.LARGE_N - 1):
        piece, = O.cut_poly(polys[k], np.zeros((4, 4), np.uint8))
        assert len(piece) == 4 and X.branch_of(piece, p) == "circle" and X.fate_of(O, piece, p) == "tap"
        seen.add(tuple(polys[k].reshape(-1).tolist()))
    assert len(seen) == 6                                                   # polyline 2300 repeats polyline 0; those past 65535 are new
    assert lines == []                                                      # every piece is a tap: n_seq = LARGE_N
    assert X.LARGE_N * 17 + 64 > 150 * 1024 and X.LARGE_N >= 9032           # past the one-wave filter
    assert len(taps) == X.LARGE_SPOTS > 2 * 1024                            # the accepted list passes 1024 twice
    assert len(set(taps)) == len(taps) and taps[-300:] == [(10 + 6 * (s % 300) + 2, 10 + 4 * (s // 300)) for s in range(X.LARGE_SPOTS - 300, X.LARGE_SPOTS)]


# ---------------------------------------------------------------- B. tiny and the tap rule
def piece_of(poly):
    piece, = O.cut_poly(poly, np.zeros((80, 80), np.uint8))
    return piece


def b_point_sets():
    out = {"tiny_" + n: piece_of(p) for n, p in X.TINY.items()}
    out.update({"thresh_" + n: piece_of(p) for n, p in X.THRESH.items()})
    out.update({"box_" + b[0]: piece_of(b[1]) for b in X.BOX})
    out.update({"odd_" + n: piece_of(X.P(p)) for n, p, _ in X.ODD})
    return out


B_SETS = b_point_sets()


@pytest.mark.parametrize("name", sorted(B_SETS))
def test_enclosing_circle_against_the_stand_in(name):
    """centre and radius as float32 bit patterns: the oracle, the independent restatement under tests/golden, and the traced restatement of cross_cases"""
    pts = B_SETS[name].reshape(-1, 2).astype(np.float32)
    (ox, oy), orad = O.min_enclosing_circle(pts)
    (sx, sy), srad = cv2_standin.minEnclosingCircle(pts)
    assert [X.bits(ox), X.bits(oy), X.bits(orad)] == [X.bits(sx), X.bits(sy), X.bits(srad)]
    if len(pts) >= 3:
        (tx, ty), trad, _ = X.mec_trace(pts)
        assert [X.bits(ox), X.bits(oy), X.bits(orad)] == [X.bits(tx), X.bits(ty), X.bits(trad)]


@pytest.mark.parametrize("name", sorted(X.TINY))
def test_tiny_case_reaches(name):
    poly = X.TINY[name]; piece = piece_of(poly); p = X.prm_of(X.tiny_case(name))
    assert X.branch_of(piece, p) == "circle" and X.fate_of(O, piece, p) == "tap"
    kept, taps = O.tiny_and_taps10([piece], X.prm_vec(p))
    assert kept == [] and len(taps) == 1
    for c, fate in X.tiny_pinned(O, name):
        assert X.branch_of(piece, X.prm_of(c)) == "circle" and X.fate_of(O, piece, X.prm_of(c)) == fate
        assert [len(v) for v in X.want(O, c)[0]] == [int(fate == "keep"), 0]
    if name.startswith("count_"):
        assert len(piece) == int(name[6:]) and same_polys([piece], [poly])
    if name.startswith("duplicates"):
        v = tl([piece])[0]
        assert len(set(v)) < len(v)
        if name == "duplicates_first_two":
            assert v[0] == v[1]
    if name in X.TINY_REACH:
        assert same_polys([piece], [poly])          # a unit walk: the piece is the walk, index for index
        lvl, adv, lane = X.TINY_REACH[name]
        finds = X.mec_trace(piece)[2]
        assert any(f[0] == lvl and f[1] == adv and lane in (None, f[2]) for f in finds), finds
        lost = X.mec_trace(piece, drop=X.TINY_REACH[name])
        assert X.bits(lost[1]) != X.bits(X.mec_trace(piece)[1])          # overlooked there, the search ends with another radius: 2 r is pinned from both sides on the device


def test_tiny_counts_and_shapes_asked_for():
    assert {2, 3, 63, 64, 65, 66, 127, 128, 129, 200} == {int(n[6:]) for n in X.TINY if n.startswith("count_")}
    ang = {}
    for n in ("three_acute", "three_right", "three_obtuse", "three_collinear"):
        a, b, c = X.TINY[n].reshape(-1, 2).astype(np.int64)
        s = sorted([int(((a - b) ** 2).sum()), int(((a - c) ** 2).sum()), int(((b - c) ** 2).sum())])
        cross = int((b - a)[0] * (c - a)[1] - (b - a)[1] * (c - a)[0])
        ang[n] = "collinear" if cross == 0 else ("acute" if s[0] + s[1] > s[2] else "right" if s[0] + s[1] == s[2] else "obtuse")
    assert ang == {"three_acute": "acute", "three_right": "right", "three_obtuse": "obtuse", "three_collinear": "collinear"}


@pytest.mark.parametrize("name", sorted(X.THRESH))
def test_thresholds_hit_exactly_and_one_step_to_either_side(name):
    piece = piece_of(X.THRESH[name])
    d = X.diameter(O, piece)
    assert float(np.nextafter(d, 0.0)) < d < float(np.nextafter(d, np.inf))
    ths = X.thresholds(O, name)
    assert len(ths) == (11 if name == "oblique" else 14)          # the axis-aligned pieces have integer perimeters
    for over, branch, fate in ths:
        p = X.prm_of(X.thresh_case(name, **over))
        assert X.branch_of(piece, p) == branch and X.fate_of(O, piece, p) == fate, over
        kept, taps = O.tiny_and_taps10([piece], X.prm_vec(p))
        assert (len(kept), len(taps)) == {"tap": (0, 1), "keep": (1, 0), "drop": (0, 0)}[fate], over


@pytest.mark.parametrize("i", range(len(X.BOX)), ids=[b[0] for b in X.BOX])
def test_bbox_shortcuts_at_their_boundaries(i):
    name, poly, over, branch, fate = X.BOX[i]
    piece = piece_of(poly); p = X.prm_of(X.box_case(i)); v = piece.reshape(-1, 2)
    ext = int(max(np.ptp(v[:, 0]), np.ptp(v[:, 1])))
    assert X.branch_of(piece, p) == branch and X.fate_of(O, piece, p) == fate
    if name.startswith("ext_equals_big"):
        assert ext == max(p["tap_diam"], p["min_keep"]) + 2
    if name == "ext_above_big":
        assert ext == max(p["tap_diam"], p["min_keep"]) + 3
    if "ext_equals_min_keep_2" in name:
        assert ext == p["min_keep"] + 2
    if "ext_below_min_keep_2" in name:
        assert ext == p["min_keep"] + 1 if "dropped" not in name else ext < p["min_keep"] + 2
    if name.startswith("many") or name == "vertices_one_too_many":
        assert len(piece) > p["tap_max_v"]
    if name.startswith("few"):
        assert len(piece) == p["tap_max_v"]
    kept, taps = O.tiny_and_taps10([piece], X.prm_vec(p))
    assert (len(kept), len(taps)) == {"tap": (0, 1), "keep": (1, 0), "drop": (0, 0)}[fate]


def test_odd_two_point_taps():
    """centres on .5 go to the even neighbour: worked by hand in cross_cases.ODD"""
    lines, taps = X.want(O, X.ODD_CASE)[0]
    assert lines == [] and taps == [t for _, _, t in X.ODD]
    for n, p, t in X.ODD:
        (cx, cy), _ = O.min_enclosing_circle(piece_of(X.P(p)).reshape(-1, 2).astype(np.float32))
        a, b = np.asarray(p, np.float64)
        assert (cx, cy) == tuple((a + b) / 2) and (cx % 1 == 0.5 or cy % 1 == 0.5), n
        assert t == (int(np.rint(cx)), int(np.rint(cy)))


# ---------------------------------------------------------------- C. paint
def paint_list():
    return [(W, H, r, g) for W, H in X.CANVASES for r in X.RADII for g in X.PAINT_GROUPS]


def test_paint_canvases_and_radii_asked_for():
    assert {W % 4 for W, _ in X.CANVASES} == {0, 1, 2, 3}
    assert {37, 64, 65, 131} <= {W for W, _ in X.CANVASES} and {29, 32, 33, 70} <= {H for _, H in X.CANVASES}
    assert X.RADII == [0, 1, 30, 61, 62]
    for r in X.RADII:
        assert X.rad_lines(dict(D_lines=float(2 * r + 1))) == r
    assert X.rad_taps(X.BASE) == 1 and X.rad_lines(X.BASE) == 0 and X.rad_taps(X.D_PRM) == 5
    W, H, r = 131, 70, 30
    g = X.paint_groups(W, H, r)
    xs = {int(p.reshape(-1, 2)[0, 0]) for p in g["touch_left_right"]}; ys = {int(p.reshape(-1, 2)[0, 1]) for p in g["touch_top_bottom"]}
    assert {-r, -r - 1, -63, -64, -65, W - 1 + r, W + r, W + 62, W + 63, W + 64} <= xs and {-r, -r - 1, -63, -64, -65, H - 1 + r, H + r, H + 62, H + 63, H + 64} <= ys
    assert {tuple(p.reshape(-1, 2)[0]) for p in g["corners_near"] + g["corners_far"]} == {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)}
    assert -1 in {int(p.reshape(-1, 2)[0, 0]) for p in g["just_outside"]} and W in {int(p.reshape(-1, 2)[0, 0]) for p in g["just_outside"]}


@pytest.mark.parametrize("W,H", X.CANVASES)
def test_paint_cases_show_their_raster_to_the_probes(W, H):
    """for every paint case: no free pixel is alone in its row AND in its column, so rows and columns together return the raster -- rebuilt here from the oracle's
    answer for the two probe layers; the painting layer stays below the stage's switch to the separable form"""
    partial = 0
    for r in X.RADII:
        for g in X.PAINT_GROUPS:
            c = X.paint_case(W, H, r, g, True)
            res, forb = X.raster_after(O, c, 1)
            assert not X.isolated_free(forb).any(), c["name"]
            assert not X.takes_separable(O, c), c["name"]
            seen = np.zeros((H, W), bool)
            for rows in (True, False):
                for p in X.want(O, X.paint_case(W, H, r, g, rows))[1][0]:
                    v = p.reshape(-1, 2); seen[v[:, 1], v[:, 0]] = True
            assert np.array_equal(seen, forb == 0), c["name"]
            partial += int(0 < int((forb != 0).sum()) < W * H)
            if g == "chains":
                v = np.concatenate([l.reshape(-1, 2) for l in res[0][0]]).astype(np.int64)
                step = np.abs(np.diff(v, axis=0)).max(1)
                assert (step == 0).any() and (np.abs(np.diff(v, axis=0)).sum(1) == 2).any()          # a repeated position, a step of sqrt(2)
                if 2 * r < min(W, H) - 10:
                    assert (step > 2 * r).any()                                                    # and a jump of more than 2 r between two polylines
    assert partial >= 12, partial


def test_paint_crowded_takes_the_separable_form_by_itself():
    for rows in (True, False):
        c = X.crowded_case(rows)
        assert X.takes_separable(O, c)
        _, forb = X.raster_after(O, c, 1)
        assert not X.isolated_free(forb).any() and 0 < int((forb != 0).sum()) < c["W"] * c["H"]


# ---------------------------------------------------------------- D. tap filter
@pytest.mark.parametrize("name", sorted(X.TAPS))
def test_tap_filter_answers_worked_by_hand(name):
    c, taps = X.TAPS[name]
    assert X.want(O, c)[-1][1] == taps


def test_tap_filter_cases_reach():
    r2 = X.rad_taps(X.D_PRM) ** 2
    assert r2 == 25
    d2 = lambda a, b: (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2
    cand = X.TAPS["exactly_r"][0]["layers"][0][1]
    assert [d2(cand[0], q) for q in cand[1:]] == [25, 25, 26, 25, 25, 25, 37]          # on the circle in five directions, and r^2 + 1
    assert d2((-2, 10), (1, 14)) == 25 and d2((60, 30), (57, 34)) == 25 and d2((30, -5), (30, 0)) == 25 and d2((33, 53), (30, 49)) == 25
    c, _ = X.TAPS["on_own_line"]
    lines, _ = X.want(O, c)[0]
    assert tl(lines) == [[(x, 30) for x in range(10, 31)]]
    c, taps = X.TAPS["given_before_line_taps"]
    from_lines = O.tiny_and_taps10([piece_of(p) for p in c["layers"][0][0]], X.prm_vec(X.prm_of(c)))[1]
    assert from_lines == [(10, 10), (40, 40), (21, 30)] and d2((12, 10), (10, 10)) <= r2 and d2((40, 45), (40, 40)) == r2


@pytest.mark.parametrize("n", X.ACCEPTED)
def test_accepted_counts(n):
    """n taps are accepted when the candidate that only the LAST of them hits is tested (slot n - 1 of the accepted list: lane 63, or lane 0 of the next 64)"""
    c, taps = X.accepted_case(n)
    cand = c["layers"][0][1]
    assert X.want(O, c)[0][1] == taps and taps[:n] == cand[:n] and len(taps) == n + 2
    d2 = lambda a, b: (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2
    assert [k for k in range(n) if d2(cand[k], cand[n + 1]) <= 25] == [n - 1] and [k for k in range(n) if d2(cand[k], cand[n + 2]) <= 25] == [n - 1]
    assert [k for k in range(n) if d2(cand[k], cand[n]) <= 25] == [0]
    assert len(cand) * 17 + 64 <= 150 * 1024          # the one-wave filter takes it


def test_tap_discs_show_to_the_probes():
    c = X.tap_stamp_case(True)
    res, forb = X.raster_after(O, c, 1)
    assert res[0][1] == c["layers"][0][1]          # all accepted, the six off the canvas included
    assert not X.isolated_free(forb).any()
    cov = forb != 0
    assert cov[0, 5] and not cov[0, 6] and cov[4, 3] and not cov[4, 4]          # (5, 0) and (3, 4) lie on the circle around (0, 0)
    assert cov[12, 0] and not cov[12, 1] and not cov[:, 0][20:29].any()          # x = -5 reaches column 0 in one pixel, x = -6 does not
    assert cov[0, 22] and not cov[0, 30:37].any() and cov[14, 44] and not cov[22:31, 44].any() and cov[37, 12] and not cov[37, 20:29].any()
    seen = np.zeros(forb.shape, bool)
    for rows in (True, False):
        for p in X.want(O, X.tap_stamp_case(rows))[1][0]:
            v = p.reshape(-1, 2); seen[v[:, 1], v[:, 0]] = True
    assert np.array_equal(seen, ~cov)


# ---------------------------------------------------------------- E. step_px
def test_step_px_matters_above_one_only():
    c = X.step_case()
    one = X.want(O, c)
    assert sum(len(l) for l, _ in one) > 10 and sum(len(t) for _, t in one) > 3
    for s in X.STEP_SAME:
        w = X.want(O, c, step_px=s)
        assert all(same_polys(a[0], b[0]) and a[1] == b[1] for a, b in zip(w, one)), s
    for s in X.STEP_ABOVE:
        w = X.want(O, c, step_px=s)
        assert not all(same_polys(a[0], b[0]) and a[1] == b[1] for a, b in zip(w, one)), s
