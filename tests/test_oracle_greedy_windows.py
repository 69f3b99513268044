"""The inputs of tests/test_gpu_greedy_windows.py do what they were chosen for, shown with the oracle alone: the restatement of the grid kernel's rounds
(greedy_window_cases.window_stats: the host's G, the cell shift, the windows r = 1, 3, 7, ..., the gap rule) picks the oracle's polyline at every step,
and along the order the inputs reach the wide rounds, candidate counts, ties, closed contours, borders and row counts named below.  CPU only."""
import pytest

from oracle import oracle as O
import greedy_cases as C
import greedy_window_cases as W
from util import same_polys


@pytest.fixture(scope="module")
def stats():
    out = {}
    for name, make in W.CASES.items():
        polys = make()
        order, _, _ = C.greedy07(polys, W.seed_index(polys))
        assert same_polys(C.apply_order(polys, order), O.sort07(polys)), name
        out[name] = (polys, W.window_stats(polys, order))          # raises where a round's winner is not the oracle's
    return out


def ended(st, pred):
    return sum(c for r, c in st["ends"].items() if pred(r))


def test_inputs_select_the_grid_kernel(stats):
    for name, (polys, st) in stats.items():
        n = len(polys)
        assert 2000 <= n <= 4000 and C.range_flags(polys) == 0 and C.selected_kernel(n, 0, False) == "grid", name
        assert st["G"] == W.host_G(n) >= 80, (name, st["G"])
        assert st["wide_rounds"] >= 10, (name, st)


def test_the_file_reaches_every_wide_round(stats):
    tot = lambda f: sum(f(st) for _, st in stats.values())
    assert tot(lambda st: ended(st, lambda r: r == 3)) >= 10 and tot(lambda st: ended(st, lambda r: r == 7)) >= 10
    assert tot(lambda st: ended(st, lambda r: r == 15)) >= 1 and tot(lambda st: ended(st, lambda r: r == 31)) >= 1 and tot(lambda st: ended(st, lambda r: r >= 63)) >= 1
    assert tot(lambda st: st["wide_over128"]) >= 1 and tot(lambda st: st["wide_ties"]) >= 1 and tot(lambda st: st["wide_closed"]) >= 1
    assert set().union(*(st["clips"] for _, st in stats.values())) == {"x0", "x1", "y0", "y1"}


def test_far_clusters(stats):
    polys, st = stats["far_clusters"]
    assert st["G"] == 88 and st["sh"] == 8                               # 256-px cells
    assert ended(st, lambda r: r >= 63) >= 3                             # every emptied cluster
    assert st["clips"] == {"x0", "x1", "y0", "y1"} and st["over64rows"] >= 1


def test_ladder(stats):
    _, st = stats["ladder"]
    assert ended(st, lambda r: r == 3) >= 10 and ended(st, lambda r: r == 7) >= 10, st["ends"]
    assert all(st["ends"].get(r, 0) >= 1 for r in (3, 7, 15, 31)), st["ends"]


def test_crowded(stats):
    _, st = stats["crowded"]
    assert st["wide_over128"] >= 10 and st["wide_over64"] - st["wide_over128"] >= 2       # three trips and more; two trips
    assert st["wide_ties"] >= 3
    assert ended(st, lambda r: r >= 7) >= 5 and ended(st, lambda r: r == 3) == 0           # reached from more than three cells away


def test_closed_in_wide_windows(stats):
    _, st = stats["closed_wide"]
    assert st["wide_closed"] >= 30                                       # closed contours entered from a wide round
    assert st["wide_far_end_nearer"] >= 10                               # ... while the far end of some unused closed contour is nearer than the winner


def test_more_than_64_rows(stats):
    _, st = stats["rows65"]
    assert st["max_rows"] > 64 and st["over64rows"] >= 2
    assert st["winner_beyond_row64"] >= 1                                # taken from the kernel's second pass over the rows
