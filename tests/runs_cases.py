"""Inputs for orip_runs_to_polys (csrc/vector_common.hip), shared by test_oracle_runs_cases.py (no GPU: shows with the oracle that every input selects what
it is built for) and test_gpu_runs_to_polys.py (runs them on the device).  The helper turns one flag byte per slot -- a stage-08 sample or a stage-10 cut
step -- into polylines: it reads the flags in tiles of T slots, 16 per lane and load, so the cases place accepted stretches, run starts and polyline starts
against the multiples of 16 and of T.

Stage 08.  Two ways to know which samples are accepted:
  * edge paths: one vertex per sample, 1 px apart, along the canvas' top edge; a tail longer than any path, so nothing is ever popped, the point hash stays
    empty and the mask is stamped only behind a polyline's last sample.  A sample is then accepted exactly when its rounded pixel lies on the canvas
    (08:158), and the path decides that slot by slot: inside stretches hang down from y = 0, outside stretches stand up from y = -1.
  * row snakes (as in test_gpu_stage08_chain.py): rows closer together than the collision radius, so a sample is dropped once the sample beside it on the row
    before has left the tail.  No position repeats, so the accepted samples are read off the oracle's cleaned pieces by position.
Stage 10.  One straight line of more than 3 T steps on a canvas 12 400 px wide; a darker layer drawn with a pen of half a pixel paints exactly the pixels of
its own lines into the forbidden raster, so slot s of the line is forbidden exactly when a darker line covers pixel (10 + s, 50)."""
import functools

import numpy as np

from oracle import oracle as O

T = 4096          # ORIP_RUN_TILE of csrc/vec_common.h: the slots one block of orip_runs_to_polys' two passes over the flags takes


def P(a):
    return np.asarray(a, np.int32).reshape(-1, 1, 2)


# ---------------------------------------------------------------- stage 08
CFG6 = dict(O.DEFAULTS, pixels_per_mm=6)          # canvas 1260 x 1782
# step 1 px; nothing leaves the tail; pieces up to 11 px across become taps (their centre shows their end points), the 12-px paths of the smallest cases do not
EDGE = dict(CFG6, dedup_sample_step=1, ignore_tail_points_intra=10 ** 7, tap_max_dim=11)
SNAKE = dict(CFG6, dedup_sample_step=1, ignore_tail_points_intra=300)
I, X = True, False          # a stretch of samples inside / outside the canvas


def edge_path(runs, x0=100, depth=1700):
    """one vertex per sample, consecutive vertices 1 px apart: `runs` is a list of (inside, count).  A stretch starts and ends on y = 0 (inside) or y = -1
    (outside), so the step to the next stretch is vertical; stretches of 40 samples and more go down (up) one column and come back in the next one,
    shorter ones run along the edge"""
    pts = []; x = x0
    for inside, cnt in runs:
        sgn, y0 = (1, 0) if inside else (-1, -1)
        left = cnt
        while left > 0:
            d = min((left - 2) // 2, depth) if left >= 40 else 0
            if d > 0:
                pts += [(x, y0 + sgn * j) for j in range(d + 1)] + [(x + 1, y0 + sgn * j) for j in range(d, -1, -1)]
                left -= 2 * d + 2; x += 1
            else:
                pts.append((x, y0)); left -= 1
            if left > 0:
                x += 1
    pts.append((pts[-1][0] + 1, pts[-1][1]))          # the resampling stops short of the end of the path (08:53-64): one vertex that is no sample
    return P(pts)


def mixed(ms):
    """stretches of many lengths, inside and outside in turn, `ms` samples in all"""
    lens = [37, 5, 1, 3, 130, 2, 700, 1, 1, 64, 15, 16, 17, 1000, 31, 33]
    runs = []; left = ms; k = 0
    while left > 0:
        n = min(lens[k % len(lens)], left)
        runs.append((k % 2 == 0, n)); left -= n; k += 1
    return runs


def rows_path(total, x0, y0, width, pitch, dx=1):
    """a path of rows `width` long, `pitch` apart, left to right and back, a point every dx px, cut off after exactly `total` px (test_gpu_stage08_chain.py; with a
    point on every pixel no sample is interpolated, so every position is an integer exactly)"""
    pts = [[x0, y0]]; left = total; r = 0
    while left > 0:
        run = min(width, left); sgn = -1 if r & 1 else 1
        xs = list(range(dx, run, dx)) + [run]
        x_start = pts[-1][0]
        pts += [[x_start + sgn * x, pts[-1][1]] for x in xs]
        left -= run
        if left > 0:
            down = min(pitch, left)
            xe, ye = pts[-1]
            pts += [[xe, ye + j] for j in range(1, down + 1)]; left -= down
        r += 1
    return P(pts)


def runs_of(acc, first):
    """[begin, end) of every run of accepted slots, by the rule of orip_runs_to_polys: a run starts at an accepted slot that starts a polyline, is slot 0,
    or follows a slot that is not accepted"""
    acc = np.asarray(acc, bool); first = np.asarray(first, bool)
    start = acc & (first | np.r_[True, ~acc[:-1]])
    b = np.flatnonzero(start)
    e = [int(s) + int(np.argmin(np.r_[(acc & ~start)[s + 1:], False])) + 1 for s in b]
    return list(zip(b.tolist(), e))


# name -> (polylines, configuration, samples of the layer, how the accepted samples are known, property of (acc, first))
def _cases08():
    c = {}
    def edge(name, polys, ms, prop):
        c[name] = (polys, EDGE, ms, "edge", prop)
    edge("ms15", [edge_path([(I, 7), (X, 1), (I, 7)])], 15, lambda a, f: runs_of(a, f) == [(0, 7), (8, 15)])
    edge("ms16", [edge_path([(X, 1), (I, 7), (X, 1), (I, 7)])], 16, lambda a, f: runs_of(a, f) == [(1, 8), (9, 16)])
    edge("ms17", [edge_path([(I, 8), (X, 1), (I, 8)])], 17, lambda a, f: runs_of(a, f) == [(0, 8), (9, 17)])
    for name, ms in (("msT-1", T - 1), ("msT", T), ("msT+1", T + 1), ("ms2T+1", 2 * T + 1), ("ms3T+5", 3 * T + 5)):
        edge(name, [edge_path(mixed(ms), x0=20)], ms, lambda a, f: 0 < a.sum() < len(a) and any(e - b == 1 for b, e in runs_of(a, f)))
    edge("stretch_over_tile_boundary", [edge_path([(X, T - 30), (I, 60), (X, 50)])], T + 80, lambda a, f: runs_of(a, f) == [(T - 30, T + 30)])
    edge("run_starts_on_tile_first_slot", [edge_path([(X, T), (I, 50), (X, 30)])], T + 80, lambda a, f: runs_of(a, f) == [(T, T + 50)] and not a[T - 1])
    edge("run_ends_on_tile_last_slot", [edge_path([(X, T - 50), (I, 50), (X, 40)])], T + 40, lambda a, f: runs_of(a, f) == [(T - 50, T)] and not a[T])
    edge("last_slot_accepted", [edge_path([(X, 40), (I, 30)])], 70, lambda a, f: a[-1] and runs_of(a, f) == [(40, 70)])
    edge("slot0_accepted", [edge_path([(I, 30), (X, 40)])], 70, lambda a, f: a[0] and runs_of(a, f) == [(0, 30)])
    # two polylines back to back, every sample accepted: only bit 1 splits them
    edge("two_polylines_in_tile", [edge_path([(I, 100)]), edge_path([(I, 60)], x0=400)], 160,
         lambda a, f: a.all() and f[100] and runs_of(a, f) == [(0, 100), (100, 160)])
    edge("two_polylines_on_tile_boundary", [edge_path([(I, T)]), edge_path([(I, 60)], x0=400)], T + 60,
         lambda a, f: a.all() and f[T] and runs_of(a, f) == [(0, T), (T, T + 60)])
    edge("isolated_singles", [edge_path([(X, 40), (I, 1), (X, 3), (I, 1), (X, 1), (I, 1), (X, 2), (I, 30), (X, 1), (I, 1)])], 81,
         lambda a, f: [e - b for b, e in runs_of(a, f)] == [1, 1, 1, 30, 1])
    edge("every_run_single", [edge_path([(X, 40)] + [(I, 1), (X, 1)] * 50)], 140, lambda a, f: a.sum() == 50 and all(e - b == 1 for b, e in runs_of(a, f)))
    edge("none_accepted", [edge_path([(X, 100)])], 100, lambda a, f: not a.any())
    edge("all_accepted", [edge_path([(I, 300)])], 300, lambda a, f: a.all() and runs_of(a, f) == [(0, 300)])
    # polylines that leave the canvas at a slant: fractional positions, accepted samples with a coordinate in (-0.5, 0)
    c["fractional_negative"] = ([P([[40, 300], [-3, 700], [35, 1100]]), P([[600, 30], [900, -4], [1200, 25]])], EDGE, None, "edge", None)
    for name, ms in (("snake2T+1", 2 * T + 1), ("snake3T+5", 3 * T + 5)):
        c[name] = ([rows_path(ms, 40, 60, 1000, 14)], SNAKE, ms, "pieces", lambda a, f: 0 < a.sum() < len(a) and any(b < T <= e - 1 for b, e in runs_of(a, f)))
    return c


CASES08 = _cases08()


@functools.lru_cache(maxsize=None)
def layer08(name):
    """the layer of a case as orip_dedup_layer's part A sees it, by the oracle alone: (S float64 [MS, 2] sample positions in processing order, first [MS]: a
    polyline starts here, acc [MS]: the sample is accepted, pieces: the oracle's cleaned pieces in order)"""
    polys, cfgd, _, how, _ = CASES08[name]
    prm = O.derived08(cfgd); W, H = O.canvas_size(cfgd)
    step = max(1.0, float(cfgd["dedup_sample_step"]))
    kept, _ = O.split_small_taps08(polys, prm)
    per = [np.float32(O.poly_perimeter(p)) for p in kept]
    order = sorted(range(len(kept)), key=lambda i: -per[i])          # stable, descending (08:520)
    mask = np.zeros((H, W), np.uint8)
    Ss, firsts, accs, pieces = [], [], [], []
    for i in order:
        a = np.asarray(kept[i]).reshape(-1, 2); n = len(a)
        if n >= 2 and (a[0] == a[n - 1]).all():
            n -= 1
        pc = O.virtual_draw08(kept[i], mask, prm)
        pieces += pc
        if n < 2:
            continue
        f = a[:n].astype(np.float32)
        S, _ = O.resample_arclen(f, bool(n > 2 and (f[0] == f[n - 1]).all()), step)
        S = np.asarray(S, np.float64)
        if len(S) < 2:
            continue
        if how == "edge":
            r = np.rint(S)
            acc = (r[:, 0] >= 0) & (r[:, 1] >= 0) & (r[:, 0] < W) & (r[:, 1] < H)
        else:          # no position repeats: a sample is accepted when a piece of its polyline holds its (integer) position
            assert (S == np.rint(S)).all() and len({tuple(p) for p in S.tolist()}) == len(S)
            have = {tuple(q) for p in pc for q in np.asarray(p).reshape(-1, 2).tolist()}
            acc = np.array([(int(x), int(y)) in have for x, y in S], bool)
        first = np.zeros(len(S), bool); first[0] = True
        Ss.append(S); firsts.append(first); accs.append(acc)
    if not Ss:
        return np.zeros((0, 2)), np.zeros(0, bool), np.zeros(0, bool), pieces
    return np.concatenate(Ss), np.concatenate(firsts), np.concatenate(accs), pieces


def pieces_of(S, acc, first):
    """what orip_runs_to_polys must return: every run of two accepted slots and more, each position truncated toward zero"""
    return [np.trunc(S[b:e]).astype(np.int32).reshape(-1, 1, 2) for b, e in runs_of(acc, first) if e - b >= 2]


def holds08(name):
    """the case selects what it is built for (asserted by the oracle test, and by the GPU test before it runs the device)"""
    _, _, ms, _, prop = CASES08[name]
    S, first, acc, pieces = layer08(name)
    want = pieces_of(S, acc, first)
    assert len(want) == len(pieces) and all(np.array_equal(np.asarray(x).reshape(-1, 2), np.asarray(y).reshape(-1, 2)) for x, y in zip(want, pieces)), name
    if ms is not None:
        assert len(S) == ms, (name, len(S))
    if prop is not None:
        assert prop(acc, first), name
    return S, first, acc


# ---------------------------------------------------------------- stage 10
CFG10 = dict(O.DEFAULTS, pixels_per_mm=10, target_width_mm=1240, target_height_mm=10, pen_width_px=0.5, color_names=["layer_dark", "layer_light"])      # canvas 12400 x 100
L10 = 3 * T + 40                                   # the line's length in px: slots 0 .. L10, slot s at (10 + s, 50)
LINE10 = P([[10, 50], [10 + L10, 50]])


def _stretch(b, e):
    """a darker line over slots [b, e) of LINE10"""
    return P([[10 + b, 50], [10 + e - 1, 50]])


CASES10 = {          # name -> (the darker layer's lines, the runs of allowed slots)
    "all_allowed": ([], [(0, L10 + 1)]),
    "all_forbidden": ([LINE10.copy()], []),
    "alternating_singles": ([P([[10 + s, 44], [10 + s, 56]]) for s in range(1, L10 + 1, 2)], [(s, s + 1) for s in range(0, L10 + 1, 2)]),
    "stripe_edges_on_tile_boundaries": ([_stretch(T - 50, T), _stretch(5000, 5100), _stretch(2 * T, 2 * T + 50)],
                                        [(0, T - 50), (T, 5000), (5100, 2 * T), (2 * T + 50, L10 + 1)]),
}


@functools.lru_cache(maxsize=None)
def layer10(name):
    """(allowed [L10 + 1]: the flags of LINE10's slots behind the darker layer, the oracle's cut pieces)"""
    dark, _ = CASES10[name]
    W, H = O.canvas_size(CFG10)
    forb = np.zeros((H, W), np.uint8)
    O.stage10_layer(dark, [], forb, O.derived10(CFG10))
    allowed = forb[50, 10:10 + L10 + 1] == 0
    return allowed, O.cut_poly(LINE10, forb, 1.0)


def holds10(name):
    _, runs = CASES10[name]
    allowed, pieces = layer10(name)
    first = np.zeros(len(allowed), bool); first[0] = True
    assert len(allowed) == L10 + 1 > 3 * T and runs_of(allowed, first) == runs, name
    # the points of a piece, as 10:160-170 forms them in float32: p0 + v * float32(k / n), truncated (the product is off by up to an ulp of k, so some points repeat)
    k = np.arange(L10 + 1, dtype=np.float64)
    qx = (np.float32(10) + np.float32(L10) * (k / L10).astype(np.float32)).astype(np.float32)
    assert (np.rint(qx) == 10 + k).all()          # the pixel a slot is tested at is exact
    want = [np.stack([np.trunc(qx[b:e]), np.full(e - b, 50.0)], 1).astype(np.int32) for b, e in runs if e - b >= 2]
    assert len(want) == len(pieces) and all(np.array_equal(x.reshape(-1, 2), np.asarray(y).reshape(-1, 2)) for x, y in zip(want, pieces)), name


def intra10(name):
    return {"layer_dark": (CASES10[name][0], []), "layer_light": ([LINE10], [])}
