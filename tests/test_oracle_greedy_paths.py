"""The inputs of tests/test_gpu_greedy_paths.py do what they were chosen for: with the oracle alone, every case of tests/greedy_cases.py has the
coordinate-range flags, and therefore the greedy kernel, that its entry names; the plain restatement of the greedy order (greedy_cases.greedy07) gives
the oracle's order, and along it every small case has steps whose smallest distance different polylines share and closed contours that are entered.
CPU only."""
import numpy as np
import pytest

from oracle import oracle as O
import greedy_cases as C
from util import same_polys


@pytest.mark.parametrize("name", list(C.CASES))
def test_flags_and_selected_kernel(name):
    seed, n, centres, spread, extra, nogrid, flags, kernel = C.CASES[name]
    polys = C.polys_of(name)
    assert len(polys) == n and all(2 <= len(p) <= 5 for p in polys)
    assert C.range_flags(polys) == flags
    assert C.selected_kernel(n, flags, nogrid) == kernel
    _, _, closed = C.ends07(polys)
    assert 0.1 * n <= closed.sum() <= 0.4 * n or n < 100 and closed.sum() >= 3


def test_every_kernel_and_thread_count_is_reached():
    assert {v[7] for v in C.CASES.values()} == {"grid", "lds", "global256", "global1024"}
    assert {(v[1], v[7]) for v in C.CASES.values()} >= {(63, "lds"), (64, "grid"), (65, "grid"), (200, "lds"), (16001, "global1024")}
    # the gates one step to either side: 64 polylines start the grid kernel, 16 000 are the last that fit the LDS store
    assert C.selected_kernel(63, 0, False) == "lds" and C.selected_kernel(64, 0, False) == "grid"
    assert C.selected_kernel(16000, 0, False) == "lds" and C.selected_kernel(16001, 0, False) == "global1024"
    assert C.selected_kernel(70, 1, False) == C.selected_kernel(70, 2, False) == C.selected_kernel(70, 3, False) == "global256"
    assert C.selected_kernel(40, 2, False) == "lds" and C.selected_kernel(40, 3, False) == "global256"


@pytest.mark.parametrize("name", C.SMALL)
def test_ties_and_closed_contours_along_the_oracles_order(name):
    polys = C.polys_of(name)
    seed_index = int(np.argmax([O.arc_length(p, True) for p in polys]))            # the first of equal maxima
    order, ties, entered = C.greedy07(polys, seed_index)
    assert same_polys(C.apply_order(polys, order), O.sort07(polys))
    assert ties >= 1 and entered >= 1, (ties, entered)
    assert any(flip for _, flip in order) and sorted(i for i, _ in order) == list(range(len(polys)))


def test_negative_cases_span_the_signed_ranges():
    for name, (lo, hi) in (("n70_negative", C.B15), ("n40_negative", C.I16)):
        s, e, _ = C.ends07(C.polys_of(name))
        xy = np.concatenate([s, e])
        assert xy.min() < lo * 0.95 and xy.max() > hi * 0.9 and xy.min() >= lo and xy.max() <= hi


def test_far_end_points_are_end_points():
    """the far coordinate of the flag cases belongs to an end point stage 07 uses (rule07: start, or the end of the open reading)"""
    for name, far in (("n70_x20000", 20000), ("n70_y-20000", -20000), ("n40_40000", 40000), ("n70_40000", 40000)):
        s, e, _ = C.ends07(C.polys_of(name))
        assert (np.concatenate([s, e]) == far).any(), name
