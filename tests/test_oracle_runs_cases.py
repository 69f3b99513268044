"""No GPU: every input of runs_cases.py selects what it is built for, shown with the oracle alone -- the sample count by the oracle's resampling, the
cleaned pieces by O.virtual_draw08 / O.cut_poly, and from them the piece boundaries at the intended slots, the single accepted slots that no piece shows,
the empty and the full layers.  test_gpu_runs_to_polys.py asserts the same before it runs the device."""
import numpy as np
import pytest

import runs_cases as R
from runs_cases import T


def test_runs_of_rule():
    """the run rule itself, on a hand-made flag list: slot 0, a gap, a polyline start inside an accepted stretch, a single, the last slot"""
    acc = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1, 0, 1, 1], bool)
    first = np.zeros(12, bool); first[[0, 5]] = True
    assert R.runs_of(acc, first) == [(0, 2), (3, 5), (5, 7), (8, 9), (10, 12)]
    assert R.runs_of(np.zeros(5, bool), np.zeros(5, bool)) == []


@pytest.mark.parametrize("name", sorted(R.CASES08))
def test_stage08_case_selects(name):
    R.holds08(name)


def test_stage08_sizes_cover_the_tile_and_the_wide_load():
    """the sample counts asked for: around one 16-flag load, around one tile, over two and three tiles with a partial last load"""
    ms = {R.CASES08[n][2] for n in R.CASES08}
    assert {15, 16, 17, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5} <= ms
    assert max(m for m in ms if m) <= 4 * T


def test_stage08_single_slots_show_in_no_piece():
    """a run of one accepted sample is dropped: the pieces hold fewer points than samples are accepted, by exactly the singles"""
    for name in ("isolated_singles", "every_run_single"):
        S, first, acc, pieces = R.layer08(name)
        singles = sum(1 for b, e in R.runs_of(acc, first) if e - b == 1)
        assert singles > 0 and sum(len(p) for p in pieces) == int(acc.sum()) - singles
    assert R.layer08("every_run_single")[3] == [] and R.layer08("none_accepted")[3] == []
    assert len(R.layer08("all_accepted")[3]) == 1 and len(R.layer08("all_accepted")[3][0]) == 300


def test_stage08_split_between_polylines_is_bit1_alone():
    """both back-to-back cases: the slot before the second polyline's first sample is accepted, so only the polyline start separates the two pieces"""
    for name, at in (("two_polylines_in_tile", 100), ("two_polylines_on_tile_boundary", T)):
        S, first, acc, pieces = R.layer08(name)
        assert acc[at - 1] and acc[at] and first[at] and first.sum() == 2
        assert [len(p) for p in pieces] == [at, 60]
    assert 100 % T != 0 and 100 % 16 != 0


def test_stage08_fractional_and_negative_positions():
    """accepted samples with fractional parts on both sides of .5 and with a coordinate in (-0.5, 0): rounding to the pixel (half to even) keeps them on the
    canvas, the point of the cleaned line truncates toward zero -- 0, where a floor would give -1"""
    R.holds08("fractional_negative")
    S, first, acc, pieces = R.layer08("fractional_negative")
    A = S[acc]; fr = np.abs(A - np.trunc(A))
    assert ((fr > 0) & (fr < 0.5)).any() and (fr > 0.5).any()
    neg = (A < 0).any(axis=1)
    assert neg.sum() >= 2 and (A[neg].min(axis=1) > -0.5).all()
    assert (~acc).any() and (S[~acc] < -0.5).any()
    pts = np.concatenate([np.asarray(p).reshape(-1, 2) for p in pieces])
    assert pts.min() == 0 and len(pts) >= int(neg.sum())


def test_snakes_drop_by_collision():
    """the row snakes: every dropped sample lies on the canvas (it is the collision test that drops it), whole stretches of rows are dropped, and an accepted
    stretch crosses the first tile boundary"""
    for name in ("snake2T+1", "snake3T+5"):
        S, first, acc = R.holds08(name)
        W, H = R.O.canvas_size(R.SNAKE)
        assert (S >= 0).all() and (S[:, 0] < W).all() and (S[:, 1] < H).all()
        runs = R.runs_of(acc, first)
        assert len(runs) >= 4 and min(e - b for b, e in runs) >= 2 and (~acc).sum() > 1000


@pytest.mark.parametrize("name", sorted(R.CASES10))
def test_stage10_case_selects(name):
    R.holds10(name)


def test_stage10_cases_are_what_they_are_called():
    assert R.layer10("all_allowed")[0].all() and len(R.layer10("all_allowed")[1]) == 1
    assert not R.layer10("all_forbidden")[0].any() and R.layer10("all_forbidden")[1] == []
    a = R.layer10("alternating_singles")[0]
    assert a[0::2].all() and not a[1::2].any() and R.layer10("alternating_singles")[1] == []
    a = R.layer10("stripe_edges_on_tile_boundaries")[0]
    assert not a[T - 1] and a[T] and a[2 * T - 1] and not a[2 * T]
