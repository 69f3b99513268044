"""Inputs for the sequential tail replay of stage 08-A (csrc/vector08a.hip: k_tail_par marks a polyline with its last unsure sample, k_tail_replay
redoes it up to there).  tests/test_oracle_tail_replay_cases.py (CPU) shows on the oracle's own samples that every case holds what it is built for;
tests/test_gpu_stage08_tail_replay.py (GPU) compares the device with the oracle.  Plain data and numpy.

All polylines are axis-parallel with integer ends, so cumulative lengths and sample distances are exact.  With a step that divides the tail length a
straight run has tails EQUAL to the threshold, which k_tail_par cannot decide (unsure).  Where a corner lies at an odd arc length and the step is 2, the
samples on either side cut it (a chord of sqrt 2): a tail with such a chord in it misses the threshold by 0.24 px at least and is sure.

A case is (id, config overrides, polylines, per polyline: what the companion asserts)."""
import numpy as np


def P(a):
    return np.asarray(a, np.int32).reshape(-1, 1, 2)


def rows(total, x0, y0, width, pitch, dx=5):
    """tests/test_gpu_stage08_chain.py: rows_path, as a point list (rows `width` long, `pitch` apart, cut off after exactly `total` px)"""
    pts = [[x0, y0]]; left = total; r = 0
    while left > 0:
        run = min(width, left); sgn = -1 if r & 1 else 1
        xs = list(range(dx, run, dx)) + [run]
        x_start = pts[-1][0]
        pts += [[x_start + sgn * x, pts[-1][1]] for x in xs]
        left -= run
        if left > 0:
            down = min(pitch, left)
            pts.append([pts[-1][0], pts[-1][1] + down]); left -= down
        r += 1
    return pts


def snake(samples, step, x0=40, y0=60, width=1000, pitch=14):
    return P(rows(samples * step, x0, y0, width, pitch))


def early_unsure(wide_px=1400, narrow_px=4600):
    """two wide rows (corners at even arc lengths 700, 714, 1414: straight tails of exactly 120 px), then narrow rows 31 px long, 14 apart (corners at odd
    arc lengths in pairs, 90 px from pair to pair: every tail of 120 px holds a cut corner)"""
    a = rows(wide_px + 14, 40, 60, 700, 14)             # ends at the foot of the second row's drop
    x, y = a[-1]
    b = rows(narrow_px, x, y, 31, 14)
    return P(a + b[1:])


def many_pops(cycles=100, run=1000):
    """`cycles` times out and back over the same 20 px (40 px of arc: the step), so that the samples of that part all lie on the start point at distance 0
    from each other, then a straight run: its fourth sample lifts the tail over the threshold and pops every sample of the first part at once"""
    pts = [[100, 100]]
    for _ in range(cycles):
        pts += [[120, 100], [100, 100]]
    pts.append([100 + run, 100])
    return P(pts)


CFG6 = dict(pixels_per_mm=6)          # canvas 1260 x 1782

# per polyline: dict(samples=, unsure= "all" (every sample from the first full tail on) | "none" | "early" (all in the first quarter, >= 2000 sure behind), pops=)
CASES = [
    ("snake_end_to_end", dict(CFG6, dedup_sample_step=2, ignore_tail_points_intra=120), [snake(3000, 2)], [dict(samples=3000, unsure="all")]),
    ("snake_step1_tail30", dict(CFG6, dedup_sample_step=1, ignore_tail_points_intra=30, collision_radius_intra_px=18), [snake(3000, 1)], [dict(samples=3000, unsure="all")]),
    ("early_unsure", dict(CFG6, dedup_sample_step=2, ignore_tail_points_intra=120), [early_unsure()], [dict(samples=3007, unsure="early")]),
    ("tail64", dict(CFG6, dedup_sample_step=2, ignore_tail_points_intra=64), [snake(3000, 2)], [dict(samples=3000, unsure="all")]),
    ("tail128", dict(CFG6, dedup_sample_step=2, ignore_tail_points_intra=128), [snake(3000, 2)], [dict(samples=3000, unsure="all")]),
    ("many_pops", dict(CFG6, dedup_sample_step=40, ignore_tail_points_intra=120, max_join_jump_px=120.0), [many_pops()], [dict(samples=125, unsure="some", pops=64)]),
    ("two_marked_one_not", dict(CFG6, dedup_sample_step=2, ignore_tail_points_intra=120),
     [snake(1500, 2, y0=60), snake(1400, 2, y0=400), P([[100, 800], [200, 800]])],
     [dict(samples=1500, unsure="all"), dict(samples=1400, unsure="all"), dict(samples=50, unsure="none")]),
]
SEQ_TOO = {"early_unsure"}          # cases that also run with ORIP_TAIL_SEQ=1
