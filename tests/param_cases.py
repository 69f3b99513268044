"""Inputs and (key, value) lists of the vector-parameter sweeps (stages 05, 08, 10, 12 away from their default pen, radius and stride settings).
tests/test_oracle_params.py (CPU) asserts on the oracle alone that every swept value matters on these inputs; tests/test_gpu_vector_params.py
(GPU) compares the device with the oracle over the same lists.  Plain data and numpy: nothing here touches the oracle or the device."""
import numpy as np


def P(a):
    return np.asarray(a, np.int32).reshape(-1, 1, 2)


# ---------------------------------------------------------------- stage 08
PPM08 = 6                    # canvas 1260 x 1782 under the default sheet
RETRACED_PPM = 10            # the retraced-paths input keeps the canvas of test_stage08_tail_simulation_both_forms

# One parameter at a time against the defaults (pen 60 / radius 30, collision radius 18 = stride 18, step 8, tail 120, jump 80, taps 25 / 160).
SWEEP08 = [
    ("hash_stride_px", 4.0), ("hash_stride_px", 6.0), ("hash_stride_px", 17.5),                      # stride below the radius: the 3 x 3 lookup misses points
    ("collision_radius_intra_px", 0.4), ("collision_radius_intra_px", 3.0), ("collision_radius_intra_px", 9.0),      # brush 1 / 6 / 18 -> stamp radius 0 / 3 / 9
    ("collision_radius_intra_px", 25.5), ("collision_radius_intra_px", 31.0),                      # brush 51 / 62 -> 25 / 31, and the default stride 18 is below them
    ("dedup_sample_step", 3), ("dedup_sample_step", 5), ("dedup_sample_step", 11),
    ("ignore_tail_points_intra", 0), ("ignore_tail_points_intra", 40), ("ignore_tail_points_intra", 300),
    ("tap_max_dim", 12), ("tap_max_dim", 40),
    ("tap_max_perimeter", 70.0), ("tap_max_perimeter", 300.0),
    ("pen_width_px", 10), ("pen_width_px", 24),                                                     # tap_diam binds only below tap_max_dim = 25
    ("pen_radius_px", 12), ("pen_radius_px", 50),                                                    # min_keep 10 / 20 against 12
]
# hash_stride_px at or above the radius, and 0 (-> max(4, radius)): every point within the radius lies in the 3 x 3 cells, whatever the cell
# size, so the result IS the default one.  The device's direct comparison (no hash at all) stands on this identity.
STRIDE_IDENTITY08 = [("hash_stride_px", 0.0), ("hash_stride_px", 18.5), ("hash_stride_px", 25.0), ("hash_stride_px", 40.0), ("hash_stride_px", 1000.0)]
# max_join_jump_px cannot change a result the device accepts.  Stage 08 splits the segments of the virtual draw, whose neighbouring points are
# neighbouring ACCEPTED samples (a rejected or off-canvas sample ends the segment): at most dedup_sample_step apart, + sqrt(2) for the truncation
# to integers, and the stage wants 2 * dedup_sample_step < max_join_jump_px.  Stage 10 splits the cut polylines, resampled every pixel: at most
# 1 + sqrt(2) apart, and the stage wants max_join_jump_px >= 4.  The device relies on it (neither stage has a split kernel), so the sweeps run
# these values and the CPU test asserts the identity instead of a difference.
JUMP_IDENTITY08 = [("max_join_jump_px", 30.0), ("max_join_jump_px", 120.0), ("max_join_jump_px", 16.5)]
# stride below radius, as a config pair: (collision radius, stride)
STRIDE_BELOW08 = [(18.0, 4.0), (18.0, 6.0), (18.0, 17.5), (9.0, 6.0)]

RANGES08 = dict(hash_stride_px=[0.0, 4.0, 6.0, 12.0, 17.5, 25.0, 40.0], collision_radius_intra_px=[3.0, 9.0, 18.0, 25.5, 31.0],
                dedup_sample_step=[3, 5, 8, 11], ignore_tail_points_intra=[0, 40, 120, 300], max_join_jump_px=[30.0, 80.0, 120.0],
                tap_max_dim=[12, 25, 40], tap_max_perimeter=[70.0, 160.0, 300.0], pen_width_px=[10, 24, 60, 62], pen_radius_px=[12, 30, 50])


def combos08(n=8, seed=808):
    """n seeded random combinations, every key drawn from RANGES08"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        out.append({k: v[int(rng.integers(0, len(v)))] for k, v in RANGES08.items()})
    return out


def _ring(cx, cy, r, n, laps=1.0):
    t = np.linspace(0.0, 2.0 * np.pi * laps, int(n * laps) + 1)
    p = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)
    return np.rint(p).astype(np.int32)


def sweep_input08(W, H, seed=500):
    """Polylines on a W x H canvas on which every value of SWEEP08 changes the oracle's stage-08 result:
      - self-crossing random walks and a few retraced ones (mask hits, hash hits, the tail rule);
      - tracks that leave the canvas and come back next to themselves (an off-canvas sample is hashed but never stamped: only _PointHash.near sees it);
      - closed rings with diameters 5 .. 70 px, some wound more than once (perimeters 60 .. 350 px), and squares of exactly 24 / 25 / 26 px (the tap tests);
      - scribbles of more than 50 vertices inside boxes of 3 .. 25 px (too many vertices for a tap: min_keep alone decides);
      - polylines whose vertices lie 20 .. 130 px apart."""
    rng = np.random.default_rng(seed)
    lim = min(W, H)
    polys = []
    for _ in range(28):
        m = int(rng.integers(2, 80))
        p = (np.cumsum(rng.integers(-22, 23, (m, 2)), axis=0) + rng.integers(50, lim - 50, 2)).astype(np.int32)
        if rng.random() < 0.25 and m > 3:
            p[-1] = p[0]
        polys.append(p)
    for _ in range(6):
        m = int(rng.integers(20, 120))
        p = (np.cumsum(rng.integers(-9, 10, (m, 2)), axis=0) + rng.integers(100, lim - 100, 2)).astype(np.int32)
        polys.append(np.concatenate([p, p[::-1], p]))
    # off-canvas and back: down outside the left / top border, back inside a few pixels away (several offsets: some within every swept radius)
    y0 = 60
    for k, (xo, xi) in enumerate([(-5, 8), (-7, 1), (-9, 14), (-2, 21), (-12, 12), (-7, 2)]):
        ya, yb = y0 + 260 * (k % 3) + 200, y0 + 260 * (k % 3) + 430
        track = np.array([[xo, ya], [xo, yb], [(xo + xi) // 2, yb + 3], [xi, yb], [xi + (k % 2), ya]], np.int32)
        polys.append(track if k < 3 else track[:, ::-1] + np.array([150, 0], np.int32))      # the last three along the top border
    # stride 17.5 against radius 18 needs two samples 17.5 .. 18 px apart with a whole cell between them and no third one nearby: an off-canvas V whose
    # tip sample lies just left of the cell border x = 105 = 6 * 17.5, and the same polyline passing below it along y = 1 or 2 (found by search on the oracle)
    for v in ([[120, -63], [105, -1], [117, -70], [355, -63], [363, 1], [65, 1]], [[94, -112], [105, -1], [117, -119], [355, -112], [361, 2], [65, 2]],
              [[101, -64], [105, -1], [110, -64], [355, -64], [355, 1], [65, 1]]):
        polys.append(np.array(v, np.int32))
    # slanted off-canvas tracks: sample positions off the integer lattice
    for k in range(6):
        a = np.array([-int(rng.integers(1, 12)), int(rng.integers(900, 1600))]); L = int(rng.integers(150, 300)); s = int(rng.integers(-40, 41))
        b = a + np.array([-int(rng.integers(0, 6)), L]); c = b + np.array([int(rng.integers(6, 30)), int(rng.integers(0, 5))]); d = a + np.array([int(rng.integers(6, 30)) + s // 8, 0])
        polys.append(np.stack([a, b, c, d]).astype(np.int32))
    # rings: diameters 5 .. 70, perimeters 60 .. 350 (laps > 1 wind the ring again)
    for k, (dia, laps) in enumerate([(5, 1), (9, 1), (12, 1), (13, 1), (18, 1), (22, 1), (24, 1), (26, 1), (31, 1), (38, 1), (44, 1), (52, 1), (59, 1), (61, 1), (70, 1),
                                      (10, 2), (16, 2), (20, 3), (24, 2), (24, 3), (30, 2), (34, 3), (30, 4), (12, 4), (22, 4)]):
        cx, cy = 90 + 110 * (k % 10), H - 420 + 120 * (k // 10)
        per_lap = max(8, min(40, int(dia * 1.2)))
        if laps > 1:
            per_lap = max(6, int(44 / laps))                 # at most 50 vertices: the vertex limit of a tap is not what decides
        polys.append(_ring(cx, cy, dia / 2.0, per_lap, laps))
    for k, side in enumerate([24, 25, 26, 12, 13, 40, 41]):
        x, y = 100 + 120 * k, H - 60
        polys.append(np.array([[x, y], [x + side, y], [x + side, y + side], [x, y + side], [x, y]], np.int32))
    # scribbles: 55 .. 90 vertices inside a box of `ext` px
    for k, ext in enumerate([3, 6, 9, 10, 11, 12, 13, 15, 17, 19, 20, 21, 23, 25]):
        m = int(rng.integers(55, 90))
        q = np.zeros((m, 2), np.int64)
        for i in range(1, m):
            q[i] = np.clip(q[i - 1] + rng.integers(-4, 5, 2), 0, ext)
        q[m // 2] = [0, 0]; q[m // 2 + 1] = [ext, ext // 2]          # the box is reached
        polys.append((q + np.array([70 + 80 * k, H - 560])).astype(np.int32))
    # far-apart vertices: gaps 20 .. 130
    gaps = rng.permutation(np.arange(22, 131, 3))                  # 37 gaps, every decade of 20 .. 130 several times
    for k in range(5):
        gap = gaps[k::5]; ang = rng.random(len(gap)) * 2 * np.pi
        p = np.cumsum(np.stack([gap * np.cos(ang), gap * np.sin(ang)], 1), axis=0) + rng.integers(300, lim - 300, 2)
        polys.append(np.rint(p).astype(np.int32))
    return [P(p) for p in polys]


def retraced_input08(W, H):
    """the input of test_stage08_tail_simulation_both_forms (retraced random walks: the tail rule decides what survives)"""
    rng = np.random.default_rng(77)
    polys = []
    for _ in range(40):
        m = int(rng.integers(20, 400))
        p = (np.cumsum(rng.integers(-9, 10, (m, 2)), axis=0) + rng.integers(100, min(W, H) - 100, 2)).astype(np.int32)
        polys.append(np.concatenate([p, p[::-1], p]).reshape(-1, 1, 2))
    return polys


# ---------------------------------------------------------------- stages 10 and 12 (the builders of tests/test_gpu_vector.py, same seeds)
def rand_polys(rng, n, lo=2, hi=40, span=8000, step=15, closed_p=0.3):
    out = []
    for _ in range(n):
        m = int(rng.integers(lo, hi))
        p = (np.cumsum(rng.integers(-step, step + 1, (m, 2)), axis=0) + rng.integers(200, span, 2)).astype(np.int32)
        if rng.random() < closed_p and m > 3:
            p[-1] = p[0]
        out.append(p.reshape(-1, 1, 2))
    return out


def _taps(a):
    return [(int(x), int(y)) for x, y in a]


NAMES10 = ["layer_dark", "layer_mid", "x_extra", "layer_light"]
SWEEP10 = [("pen_width_px", 24), ("pen_width_px", 61), ("pen_width_px", 62)]
JUMP_IDENTITY10 = [("max_join_jump_px", 4.0), ("max_join_jump_px", 30.0), ("max_join_jump_px", 120.0)]      # see JUMP_IDENTITY08


# (D_lines, D_taps) through the ABI struct: the config ties both to 2 * pen_width_px.  400 -> tap radius exactly 200, the largest the stage takes.
STRUCT10 = [(120.0, 400.0), (60.0, 121.0), (124.0, 30.0), (1.0, 3.0)]


def stage10_with(O, intra, cfgd, prm):
    """oracle.stage10 with the parameter block given (oracle.stage10 derives it from the config)"""
    W, H = O.canvas_size(cfgd)
    forbidden = np.zeros((H, W), np.uint8)
    out = {}
    for name in sorted(list(cfgd["color_names"]), key=O.darkness_rank10):
        lines_in, taps_in = intra.get(name, ([], []))
        out[name] = O.stage10_layer(lines_in, taps_in, forbidden, prm)
    return out


def random_input10():
    """(config overrides, intra) of test_stage10_random_vs_oracle: canvas 1680 x 2376"""
    rng = np.random.default_rng(5)
    intra = {}
    for n in NAMES10:
        lines = rand_polys(rng, 60, lo=2, hi=25, span=1500, step=40, closed_p=0.0)
        intra[n] = (lines, _taps(rng.integers(-30, 1700, (25, 2))))
    return dict(pixels_per_mm=8, color_names=list(NAMES10)), intra


def edge_input10():
    """(config overrides, intra) of test_stage10_edge_cases: a layer without lines, one with taps only, one repeating the darkest layer's lines"""
    rng = np.random.default_rng(12)
    base = rand_polys(rng, 30, lo=2, hi=25, span=1100, step=40, closed_p=0.0)
    intra = {"layer_dark": (base, _taps(rng.integers(0, 1200, (10, 2)))),
             "layer_mid": ([], []),
             "x_extra": ([], _taps(rng.integers(0, 1200, (15, 2)))),
             "layer_light": ([p.copy() for p in base] + rand_polys(rng, 5, lo=2, hi=25, span=1100, step=40, closed_p=0.0), [])}
    return dict(pixels_per_mm=6, color_names=list(NAMES10)), intra


SWEEP12 = [("pen_width_px", 81), ("pen_width_px", 200), ("pen_width_px", 1000)]      # R_insert 81 / 200 / 1000
PEN12 = [60, 81, 200, 1000]                                                            # 60 is the default: R_insert 80, the control
CASES12 = [(0, 7), (9, 0), (300, 120), (1, 1), (60, 1500), (0, 900), (40, 2500, 40000)]      # the cases of test_stage12_random_vs_oracle
SENSITIVE12 = (60, 1500)                                                               # the case the CPU test asserts the difference on


def input12(case):
    rng = np.random.default_rng(case[0] + case[1])
    span = case[2] if len(case) > 2 else 3000
    lines = rand_polys(rng, case[0], lo=2, hi=12, span=span, step=25, closed_p=0.0)
    return lines, _taps(rng.integers(0, span, (case[1], 2)))


# ---------------------------------------------------------------- stage 05
# (name, config overrides, (w_src, h_src)): what decides offsets and scale
CASES05 = [
    ("negative_margins", dict(pixels_per_mm=4, margin_left_mm=-7.0, margin_top_mm=-0.2, margin_right_mm=-30.0, margin_bottom_mm=3.0), (96, 120)),
    ("margins_beyond_sheet", dict(pixels_per_mm=4, margin_left_mm=150.0, margin_right_mm=100.0, margin_top_mm=200.0, margin_bottom_mm=100.0), (64, 64)),
    ("margins_beyond_width_only", dict(pixels_per_mm=4, margin_left_mm=150.0, margin_right_mm=100.0), (64, 64)),
    ("half_products", dict(pixels_per_mm=5, margin_left_mm=2.5, margin_right_mm=0.5, margin_top_mm=1.5, margin_bottom_mm=3.5, target_width_mm=100.5, target_height_mm=140.5), (80, 110)),
    ("half_products_ppm7", dict(pixels_per_mm=7, margin_left_mm=0.5, margin_right_mm=1.5, margin_top_mm=2.5, margin_bottom_mm=4.5, target_width_mm=90.5, target_height_mm=60.5), (200, 90)),
    ("width_binds", dict(pixels_per_mm=6), (400, 100)),
    ("height_binds", dict(pixels_per_mm=6), (100, 400)),
    ("one_pixel_wide", dict(pixels_per_mm=6), (1, 300)),
    ("one_pixel_high", dict(pixels_per_mm=6), (300, 1)),
    ("landscape_sheet", dict(pixels_per_mm=8, target_width_mm=297, target_height_mm=210, margin_left_mm=12.0, margin_right_mm=3.0, margin_top_mm=25.0, margin_bottom_mm=0.0), (640, 360)),
    ("landscape_a5_asymmetric", dict(pixels_per_mm=10, target_width_mm=210, target_height_mm=148, margin_left_mm=5.0, margin_right_mm=20.0, margin_top_mm=0.0, margin_bottom_mm=33.0), (333, 500)),
]


def contours05(w_src, h_src, seed):
    """seeded contours inside a w_src x h_src image; the corners are always there"""
    rng = np.random.default_rng(seed)
    out = [P([[0, 0], [w_src - 1, 0], [w_src - 1, h_src - 1], [0, h_src - 1], [0, 0]])]
    for _ in range(40):
        m = int(rng.integers(1, 60))
        out.append(P(np.stack([rng.integers(0, w_src, m), rng.integers(0, h_src, m)], 1)))
    return out


# ---------------------------------------------------------------- resident chain
CFG_C = dict(pixels_per_mm=4, pen_width_px=24, pen_radius_px=12, collision_radius_intra_px=9.0, hash_stride_px=6.0, dedup_sample_step=3,
             ignore_tail_points_intra=40, max_join_jump_px=30.0, tap_max_dim=12, tap_max_perimeter=70.0, margin_left_mm=5.0, margin_right_mm=20.0,
             margin_top_mm=0.0, margin_bottom_mm=33.0, target_width_mm=150, target_height_mm=100)
CFG_D = dict(pixels_per_mm=5, pen_width_px=62, pen_radius_px=20, collision_radius_intra_px=25.5, hash_stride_px=40.0, dedup_sample_step=11,
             ignore_tail_points_intra=300, max_join_jump_px=120.0, tap_max_dim=40, tap_max_perimeter=300.0, margin_left_mm=0.0, margin_right_mm=0.0)
CFG_E = dict(pixels_per_mm=8, pen_width_px=40, pen_radius_px=45, collision_radius_intra_px=12.5, hash_stride_px=5.0, dedup_sample_step=5,
             ignore_tail_points_intra=80, max_join_jump_px=50.0, tap_max_dim=18, tap_max_perimeter=110.0, margin_left_mm=2.5, margin_right_mm=14.0,
             margin_top_mm=21.5, margin_bottom_mm=4.0, target_width_mm=148, target_height_mm=210)
# (name, overrides, (H, W, K, seed) of the synthetic image)
CHAIN = [("c", CFG_C, (160, 192, 4, 31)), ("d", CFG_D, (176, 144, 4, 32)), ("e", CFG_E, (200, 160, 5, 33))]
