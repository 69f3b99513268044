"""No GPU: every input of capsule_cases.py does what it is built for, shown with the oracle alone -- the repeated capsules lie where the case says
(in the chunk of their first occurrence, in a later chunk, beyond 65 536 samples, behind a lead of a given sample count, in another polyline, across
samples off the canvas), the expected result drops lap 2, and lap 2 is dropped by the stamps of lap 1 alone: on a canvas without them it stays."""
import numpy as np
import pytest

import capsule_cases as C
from capsule_cases import CHUNK, STEP
from oracle import oracle as O


def n_pts(segs):
    return sum(len(s) for s in segs)


def draw_in_turn(polys):
    """the accepted pieces of every polyline, the canvas going from one to the next as in 08:640-665"""
    W, H = O.canvas_size(C.CFG); mask = np.zeros((H, W), np.uint8); prm = O.derived08(C.CFG)
    return [O.virtual_draw08(p, mask, prm) for p in polys]


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_order_and_sample_counts(name):
    polys = C.CASES[name]
    per = [O.poly_perimeter(p) for p in polys]
    assert per == sorted(per, reverse=True) and len(set(per)) == len(per)
    assert [len(S) for S in C.samples(name)] == [C.n_samples(p) for p in polys]


def test_repeats_in_the_chunk_of_their_first_occurrence():
    reps = C.first_and_repeats("ring400_3laps")
    same = [v for v in reps.values() if v[0] // CHUNK == v[1] // CHUNK]
    assert len(same) > 150 and all(len(v) == 2 and v[1] - v[0] == 801 for v in reps.values())


def test_repeats_in_a_later_chunk_of_the_range():
    reps = C.first_and_repeats("ring1400_3laps")
    assert len(reps) > 900 and all(v[1] - v[0] == 2801 and v[1] // CHUNK > v[0] // CHUNK and v[1] < 4096 for v in reps.values())


def test_repeats_beyond_the_largest_range():
    reps = C.first_and_repeats("ring1400_50laps")
    assert sum(len(S) for S in C.samples("ring1400_50laps")) > 65536 + 2801
    far = [v for v in reps.values() if v[0] < 2801 and v[-1] >= 65536]
    assert len(far) > 1000 and all(len(v) >= 24 for v in far)


@pytest.mark.parametrize("name", sorted(n for n in C.CASES if n.startswith("lead")))
def test_ring_starts_where_the_lead_ends(name):
    n = int(name[4:name.index("_")])
    S = C.samples(name)
    assert len(S[0]) == n
    reps = C.first_and_repeats(name)
    assert len(reps) > 200 and min(v[0] for v in reps.values()) == n + 1          # the ring's first sample has no capsule; the lead repeats none
    assert {n % CHUNK for n in (1023, 1024, 1025, 8191, 8192, 8193, 16383, 16384, 16385)} == {1023, 0, 1}


def test_repeats_across_polylines():
    S = C.samples("two_over_one_ring"); n0 = len(S[0])
    reps = C.first_and_repeats("two_over_one_ring")
    across = [v for v in reps.values() if v[0] < n0 <= v[-1]]
    assert len(across) > 2500 and n0 + len(S[1]) > 4096 + 2801


def test_off_canvas_gap():
    keys = C.capsule_keys("ring_leaves_canvas")
    assert sum(k is None for k in keys) > 300 and len(C.first_and_repeats("ring_leaves_canvas")) > 150
    a = np.rint(C.samples("ring_leaves_canvas")[0])
    assert (a[:, 0] < 0).any() and (a[:, 0] >= 0).any()


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_expected_result_drops_lap_2(name):
    i, lap = C.ring_of(name)
    segs = draw_in_turn(C.CASES[name])
    kept = n_pts(segs[i])
    on = 1.0 if name != "ring_leaves_canvas" else 0.4
    assert on * 0.9 * lap <= kept <= lap + 16, (kept, lap)          # lap 1 stays; every later lap goes
    if name == "two_over_one_ring":
        assert n_pts(segs[1]) <= 16
    assert C.expected(name)[0]


@pytest.mark.parametrize("ring", [C.RING_S, C.RING_A, C.RING_B, (-150, 100, 500, 301)])
def test_lap_2_is_dropped_by_the_stamps_of_lap_1_alone(ring):
    """lap 2 on its own (a path that starts 2 px along the first edge), on an empty canvas and on the canvas lap 1 leaves: the point hash is per call, so only
    the stamps differ"""
    x0, y0, w, h = ring; lap = 2 * (w + h) / STEP
    W, H = O.canvas_size(C.CFG); prm = O.derived08(C.CFG)
    lap1 = C.P([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]])
    lap2 = C.P([[x0 + 2, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h], [x0, y0]])
    on = 1.0 if x0 >= 0 else 0.4
    empty = np.zeros((H, W), np.uint8)
    assert n_pts(O.virtual_draw08(lap2, empty, prm)) >= on * 0.95 * lap
    mask = np.zeros((H, W), np.uint8)
    O.virtual_draw08(lap1, mask, prm)
    assert n_pts(O.virtual_draw08(lap2, mask, prm)) <= h / STEP + 8          # (lap1 lacks its last edge: h px)
