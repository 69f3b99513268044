"""Stage 10 (csrc/vector10.hip) on the device at its edges: the cases of cross_cases.py through the ABI struct (set_polys / set_taps, orip_dedup_cross with an
orip_params10 of the case's own, get_polys / get_taps) against the oracle run with the same parameter block.  Every comparison is exact: the lines point for point
and in travel order, the taps and their order.  tests/test_oracle_cross_cases.py shows on the CPU what every case reaches -- which branch of k_tiny_taps10, which lane
of which 64-wide search of the enclosing circle, which slot of the accepted-tap list, which form of the paint -- and pins the hand-worked answers used here.

Both entries are run: orip_dedup_cross, and orip_dedup_cross_layer_deferred followed by the reorder in orip_plot_order (the paint then sees the kept lines in cut
order instead of travel order).

The paint cases observe the forbidden raster a layer leaves through a probe layer (see cross_cases.py): once with a probe along every row and once along every
column.  A free pixel with no free neighbour in its row and none in its column would show in neither; the CPU file asserts that no case has one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import cross_cases as X
from util import same_polys

ENTRIES = ["direct", "deferred"]


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def struct_of(p):
    from orip import lib as L
    return L.Params10(**{k: (int(p[k]) if k in ("tap_max_v", "W", "H") else float(p[k])) for k in X.FIELDS})


def run(dev, c, entry="direct", **over):
    from orip import lib as L
    n = len(c["layers"])
    for l, (lines, taps) in enumerate(c["layers"]):
        dev.set_polys(L.SLOT_LINES_INTRA, l, lines); dev.set_taps(L.TAPS_INTRA, l, taps)
    prm = struct_of(X.prm_of(c, **over))
    if entry == "direct":
        dev.dedup_cross(list(range(n)), prm)
    else:
        dev.dedup_cross_begin(prm)
        for l in range(n):
            dev.dedup_cross_layer(l, defer_reorder=True)
        for l in range(n):
            dev.plot_order(l, 80.0)
    return [(dev.get_polys(L.SLOT_LINES_CROSS, l), dev.get_taps(L.TAPS_CROSS, l)) for l in range(n)]


_WANT = {}


def want(c, **over):
    key = (c["name"], tuple(sorted(over.items())))
    if key not in _WANT:
        _WANT[key] = X.want(O, c, **over)
    return _WANT[key]


def same(got, wnt, what):
    assert len(got) == len(wnt)
    for l, (g, w) in enumerate(zip(got, wnt)):
        assert g[1] == w[1], (what, l, "taps")
        assert same_polys(g[0], w[0]), (what, l, "lines")


def tl(polys):
    return [[tuple(int(v) for v in q) for q in np.asarray(p).reshape(-1, 2)] for p in polys]


def _env(monkeypatch, name, on):
    if on:
        monkeypatch.setenv(name, "1")
    else:
        monkeypatch.delenv(name, raising=False)


SMALL = X.small_cases()


# ---------------------------------------------------------------- A, B, D: every small case, both entries
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_case(dev, monkeypatch, name, entry):
    _env(monkeypatch, "ORIP_PAINT_SEPARABLE", False); _env(monkeypatch, "ORIP_TAPS_1WG", False)
    c = SMALL[name]
    same(run(dev, c, entry), want(c), name)


@pytest.mark.parametrize("entry", ENTRIES)
def test_answers_worked_by_hand(dev, monkeypatch, entry):
    """the device against the literals themselves: the rounding triple, the runs of 1 and 2, the odd two-point taps, the taps exactly r apart"""
    _env(monkeypatch, "ORIP_PAINT_SEPARABLE", False); _env(monkeypatch, "ORIP_TAPS_1WG", False)
    for name, lit in X.CUT_LITERAL.items():
        assert tl(run(dev, X.CUT[name], entry)[-1][0]) == lit, name
    lines, taps = run(dev, X.ODD_CASE, entry)[0]
    assert lines == [] and taps == [t for _, _, t in X.ODD]
    for name, (c, lit) in X.TAPS.items():
        assert run(dev, c, entry)[-1][1] == lit, name


@pytest.mark.parametrize("sequential", [False, True], ids=["wave", "one_workgroup"])
@pytest.mark.parametrize("name", sorted(X.TAPS) + ["accepted_%d" % n for n in X.ACCEPTED])
def test_tap_filter_both_kernels(dev, monkeypatch, name, sequential):
    """k_taps_wave (the list's second and third chunk of 64) and, under the existing switch, k_taps_sequential on the same small cases"""
    _env(monkeypatch, "ORIP_PAINT_SEPARABLE", False); _env(monkeypatch, "ORIP_TAPS_1WG", sequential)
    c, lit = X.TAPS[name] if name in X.TAPS else X.accepted_case(int(name[9:]))
    got = run(dev, c)
    assert got[-1][1] == lit
    same(got, want(c), name)


@pytest.mark.parametrize("name", sorted(X.TINY))
def test_tiny_radius_held_from_both_sides(dev, monkeypatch, name):
    """as a tap a piece shows only its rounded centre; with min_keep at the oracle's 2 r it must be kept and one ulp above dropped, so the radius is the oracle's"""
    _env(monkeypatch, "ORIP_PAINT_SEPARABLE", False); _env(monkeypatch, "ORIP_TAPS_1WG", False)
    for c, fate in X.tiny_pinned(O, name):
        w = X.want(O, c)
        assert [len(v) for v in w[0]] == [int(fate == "keep"), 0]
        same(run(dev, c), w, (name, fate))


@pytest.mark.parametrize("name", sorted(X.THRESH))
def test_thresholds(dev, monkeypatch, name):
    """tap_diam, min_keep at 2 r exactly and one ulp to either side; tap_max_per at the integer perimeter and half a pixel below; tap_max_v at n and n - 1"""
    _env(monkeypatch, "ORIP_PAINT_SEPARABLE", False); _env(monkeypatch, "ORIP_TAPS_1WG", False)
    for over, _, fate in X.thresholds(O, name):
        c = X.thresh_case(name, **over)
        lines, taps = X.want(O, c)[0]
        assert (len(lines), len(taps)) == {"tap": (0, 1), "keep": (1, 0), "drop": (0, 0)}[fate]
        same(run(dev, c), [(lines, taps)], (name, over))


# ---------------------------------------------------------------- the large layer
def test_large_layer(dev, monkeypatch):
    """65 836 polylines (the grids of k_cut_counts and k_tiny_taps10 come round again), all of them taps: n_seq past the one-wave filter, so k_taps_sequential by
    itself, with 2 600 accepted taps (its 1024 threads come round twice)"""
    _env(monkeypatch, "ORIP_PAINT_SEPARABLE", False); _env(monkeypatch, "ORIP_TAPS_1WG", False)
    c = X.large_case()
    w = want(c)
    assert w[0][0] == [] and len(w[0][1]) == X.LARGE_SPOTS
    same(run(dev, c), w, "large layer")


# ---------------------------------------------------------------- C. paint
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("separable", [False, True], ids=["discs", "separable"])
@pytest.mark.parametrize("W,H", X.CANVASES)
def test_paint(dev, monkeypatch, W, H, separable, entry):
    """radii 0, 1, 30, 61, 62; vertices at the corners, just outside, at -r and -r - 1, around the edge of the 64-px seed pad; chains with a repeated position, steps of
    sqrt(2) and a jump between polylines.  What the painting layer leaves is read back by the probe layer, along the rows and along the columns"""
    _env(monkeypatch, "ORIP_PAINT_SEPARABLE", separable); _env(monkeypatch, "ORIP_TAPS_1WG", False)
    for r in X.RADII:
        for g in X.PAINT_GROUPS:
            for rows in (True, False):
                c = X.paint_case(W, H, r, g, rows)
                same(run(dev, c, entry), want(c), c["name"])


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("rows", [True, False], ids=["rows", "columns"])
def test_paint_crowded_canvas_takes_the_separable_form(dev, monkeypatch, rows, entry):
    _env(monkeypatch, "ORIP_PAINT_SEPARABLE", False); _env(monkeypatch, "ORIP_TAPS_1WG", False)
    c = X.crowded_case(rows)
    assert X.takes_separable(O, c)
    same(run(dev, c, entry), want(c), c["name"])


# ---------------------------------------------------------------- E. step_px
@pytest.mark.parametrize("step", X.STEP_SAME)
def test_step_px_up_to_one(dev, monkeypatch, step):
    _env(monkeypatch, "ORIP_PAINT_SEPARABLE", False); _env(monkeypatch, "ORIP_TAPS_1WG", False)
    c = X.step_case()
    same(run(dev, c, step_px=step), want(c, step_px=step), step)
    same(run(dev, c, step_px=step), want(c), (step, "is the answer of step 1"))


@pytest.mark.parametrize("step", X.STEP_ABOVE)
def test_refusal_step_px_above_one(dev, monkeypatch, step):
    """a step the stage does not honour is refused by orip_dedup_cross_begin, by name, and the context goes on working"""
    from orip.device import OripError
    _env(monkeypatch, "ORIP_PAINT_SEPARABLE", False); _env(monkeypatch, "ORIP_TAPS_1WG", False)
    c = X.step_case()
    with pytest.raises(OripError, match=r"step_px"):
        run(dev, c, step_px=step)
    with pytest.raises(OripError, match=r"step_px"):
        dev.dedup_cross_begin(struct_of(X.prm_of(c, step_px=step)))
    same(run(dev, c), want(c), "a good call after the refusal")
