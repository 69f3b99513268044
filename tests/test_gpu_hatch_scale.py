"""The fill (csrc/fill.hip), the stipple (csrc/gcode_stipple.hip) and the hatch link (csrc/gcode_link.hip) on the GPU on the cases of
tests/hatch_scale_cases.py, against their doubles, by equality and without tolerance -- segments, dots, groups, strokes, members and every count: the capped
grids of k_fl_sample / k_fl_scatter, k_st_test / k_st_emit and k_hl_elig in their second and third pass, with the scans behind them longer than 65 536 words;
the stipple's occlusion in its second and third batch of 64 shapes and at its early end; the hatch link's pointer jumping over a chain of 2 500 lines.  Then,
for all three: the largest case twice, a small case directly behind the largest, and the fill's resident form past the cap.
tests/test_hatch_scale_host.py shows that each case reaches what it is named after."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fill_cases as FC
import fill_double as FD
import hatch_link_cases as LC
import hatch_link_double as LD
import hatch_scale_cases as HS
import stipple_cases as SC
import stipple_double as SD

WANT = {}


def want(kind, name):
    """the double's answer, computed once and left unchanged"""
    if (kind, name) not in WANT:
        if kind == "fill":
            WANT[kind, name] = FD.fill_mask_numpy(*FC.args(HS.fill_cases()[name]))
        elif kind == "stipple":
            WANT[kind, name] = SD.stipple(*SC.args(HS.stipple_cases()[name]))
        else:
            WANT[kind, name] = LD.hatch_link(*LC.args(HS.link_cases()[name]))
    return WANT[kind, name]


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def equal_fill(got, exp):
    assert got[0].dtype == np.int32 and got[0].shape == exp[0].shape and got[1] == exp[1], (got[1], exp[1])
    assert np.array_equal(got[0], exp[0]), np.nonzero((got[0] != exp[0]).any(1))[0][:8]


def equal_stipple(got, exp):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2] == exp[2], (got[2], exp[2])
    assert got[0].shape == exp[0].shape and got[1].shape == exp[1].shape
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), np.nonzero((got[0] != exp[0]).any(1) | (got[1] != exp[1]))[0][:8]


def equal_link(got, exp):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int64 and got[3].dtype == np.int32
    assert got[4] == exp[4], (got[4], exp[4])
    for k, (a, b) in enumerate(zip(got[:4], exp[:4])):
        assert a.shape == b.shape and np.array_equal(a, b), (k, a[:8], b[:8])


# ================================================================================================ fill
@pytest.mark.parametrize("name", sorted(HS.FILL_UNITS))
def test_fill(dev, name):
    c = HS.fill_cases()[name]
    got = dev.fill_mask(*FC.args(c))
    equal_fill(got, want("fill", name))
    assert got[1]["lines"] > 17000 and got[1]["runs"] == got[1]["short"] + got[1]["segments"]


@pytest.mark.parametrize("name", HS.CLOSED_FORM)
def test_fill_closed_form(dev, name):
    """the second, independent answer at u = (4096, 0)"""
    seg, runs, short = FC.rows_closed_form(HS.fill_cases()[name])
    got, st = dev.fill_mask(*FC.args(HS.fill_cases()[name]))
    assert np.array_equal(got, seg) and (st["runs"], st["short"], st["segments"]) == (runs, short, len(seg))


def test_fill_resident_form_past_the_cap(dev):
    c = HS.fill_cases()["rows_two_passes"]
    masks = np.stack([HS.random_mask(*c["mask"].shape, seed=9, p=0.3), c["mask"]])
    rest = FC.args(c)[1:]
    dev.set_masks(masks)
    got = dev.fill_mask(None, *rest, layer=1)
    equal_fill(got, want("fill", "rows_two_passes"))
    equal_fill(got, dev.fill_mask(c["mask"], *rest))
    other = dev.fill_mask(None, *rest, layer=0)
    equal_fill(other, FD.fill_mask_numpy(masks[0], *rest))
    for l in range(2):
        assert np.array_equal(dev.get_mask(l), masks[l])


# ================================================================================================ stipple
@pytest.mark.parametrize("name", sorted(HS.STIPPLE_UNITS))
def test_stipple(dev, name):
    equal_stipple(dev.gcode_stipple(*SC.args(HS.stipple_cases()[name])), want("stipple", name))


@pytest.mark.parametrize("k", sorted(HS.COVER_AT))
def test_stipple_hidden_by_one_shape_of_batch(dev, k):
    """the same drawing without the one shape that hides: nothing is hidden, and the dots that come back are the 144 inside it"""
    c = HS.stipple_cases()[f"hidden_by_batch_{k}"]
    xy, grp, st = dev.gcode_stipple(*SC.args(c))
    bare = dev.gcode_stipple(*SC.args(HS.without(c, HS.COVER_AT[k])))
    assert st["hidden"] == 144 and bare[2]["hidden"] == 0 and int((bare[1] == 0).sum()) - int((grp == 0).sum()) == 144


# ================================================================================================ hatch link
@pytest.mark.parametrize("name", sorted(HS.LINK_UNITS))
def test_link(dev, name):
    exp = want("link", name)
    got = dev.gcode_hatch_link(*LC.args(HS.link_cases()[name]))
    equal_link(got, exp)
    f_off, f_pts = dev.gcode_steps_fetch(len(exp[0]) - 1, len(exp[1]))                   # the result is the resident list
    assert np.array_equal(f_off, exp[0]) and np.array_equal(f_pts, exp[1])


def test_link_consequences_on_the_tall_u(dev):
    LC.check_consequences(HS.link_cases()["tall_u"], dev.gcode_hatch_link(*LC.args(HS.link_cases()["tall_u"])))


# ================================================================================================ all three
RUN = {
    "fill": (lambda d, c: d.fill_mask(*FC.args(c)), HS.fill_cases, FC.cases, equal_fill, lambda c: FD.fill_mask(*FC.args(c))),
    "stipple": (lambda d, c: d.gcode_stipple(*SC.args(c)), HS.stipple_cases, SC.cases, equal_stipple, lambda c: SD.stipple(*SC.args(c))),
    "link": (lambda d, c: d.gcode_hatch_link(*LC.args(c)), HS.link_cases, LC.cases, equal_link, lambda c: LD.hatch_link(*LC.args(c))),
}


@pytest.mark.parametrize("kind", sorted(RUN))
def test_repeatable(dev, kind):
    run, large, _, equal, _ = RUN[kind]
    c = large()[HS.LARGEST[kind]]
    a, b = run(dev, c), run(dev, c)
    assert a[-1] == b[-1]
    for x, y in zip(a[:-1], b[:-1]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    equal(a, want(kind, HS.LARGEST[kind]))


@pytest.mark.parametrize("kind", sorted(RUN))
def test_small_after_large(dev, kind):
    """the scratch is larger than the small call needs and full of the large call's words: the answer is the small case's"""
    run, large, small, equal, double = RUN[kind]
    equal(run(dev, large()[HS.LARGEST[kind]]), want(kind, HS.LARGEST[kind]))
    c = small()[HS.SMALL[kind]]
    equal(run(dev, c), double(c))
