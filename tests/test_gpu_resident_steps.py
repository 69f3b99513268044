"""The resident step polylines between the calls that write them (csrc/orip_ctx.h states the contract): what orip_gcode_to_steps, orip_gcode_to_steps_clip,
orip_gcode_merge and orip_gcode_simplify leave behind after a bad argument, after an explicit upload and after n == 0, and when the sources still name
the polylines.  The drawing is the one of test_gpu_simplify.py's resident form: six paths in mm that become five polylines of fourteen points.  Every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAP = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=1.0, W=4000, H=4000, invert_y=0)
BAD_MAP = dict(MAP, W=0)
RECT = (0, 0, 3999, 3999)
LISTS = [[(5, 5), (9, 9)], [(9, 9), (20, 20)], [(30, 30), (30, 30.2)], [(20, 20), (26, 26), (26, 40)], [(40, 40), (45, 40), (50, 40), (50, 45), (50, 60)], [(70, 70), (80, 75)]]
OFF_MM = np.concatenate([[0], np.cumsum([len(p) for p in LISTS])]).astype(np.int64)
PTS_MM = np.asarray([q for p in LISTS for q in p], np.float64)
SOURCES = [0, 1, 3, 4, 5]                                                     # the third path rounds to one point and is dropped
EMPTY = (np.zeros(1, np.int64), np.zeros((0, 2), np.int32))


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def steps(dev):
    """the conversion's answer, computed once and only read"""
    off, pts = dev.gcode_to_steps(OFF_MM, PTS_MM, MAP)
    assert len(off) - 1 == 5 and len(pts) == 14
    return off, pts


def convert(dev, steps):
    """a good conversion: the same polylines, and the sources name them"""
    off, pts = dev.gcode_to_steps(OFF_MM, PTS_MM, MAP)
    assert np.array_equal(off, steps[0]) and np.array_equal(pts, steps[1])
    assert dev.gcode_steps_source(5).tolist() == SOURCES


def fails(call, *words):
    from orip.device import OripError
    with pytest.raises(OripError) as e:
        call()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_a_failed_conversion_drops_the_list(dev, steps):
    convert(dev, steps)
    fails(lambda: dev.gcode_to_steps(OFF_MM, PTS_MM, BAD_MAP), "orip_gcode_to_steps", "target size")
    fails(lambda: dev.gcode_steps_fetch(5, 14), "no step polylines")
    fails(lambda: dev.gcode_steps_source(5), "no step polylines")
    convert(dev, steps)


def test_a_refused_clip_leaves_the_list(dev, steps):
    convert(dev, steps)
    fails(lambda: dev.gcode_to_steps_clip(OFF_MM, PTS_MM, BAD_MAP, RECT), "orip_gcode_to_steps_clip", "target size")
    off, pts = dev.gcode_steps_fetch(5, 14)
    assert np.array_equal(off, steps[0]) and np.array_equal(pts, steps[1])
    assert dev.gcode_steps_source(5).tolist() == SOURCES
    convert(dev, steps)


def test_an_explicit_merge_ends_the_sources(dev, steps):
    convert(dev, steps)
    out = dev.gcode_merge(steps[0], steps[1], None, 1, False)
    assert out[5]["paths_out"] == 3
    fails(lambda: dev.gcode_steps_source(3), "merged")
    convert(dev, steps)


def test_an_explicit_simplify_of_as_many_keeps_the_sources(dev, steps):
    convert(dev, steps)
    off, pts, kept, st = dev.gcode_simplify(steps[0], steps[1], 0)
    assert st["paths"] == 5 and st["points_in"] == 14 and len(off) == 6
    assert dev.gcode_steps_source(5).tolist() == SOURCES
    f_off, f_pts = dev.gcode_steps_fetch(5, len(pts))
    assert np.array_equal(f_off, off) and np.array_equal(f_pts, pts)
    convert(dev, steps)


def test_an_explicit_simplify_of_another_count_ends_the_sources(dev, steps):
    convert(dev, steps)
    off4, pts4 = steps[0][:5], steps[1][:int(steps[0][4])]
    off, pts, kept, st = dev.gcode_simplify(off4, pts4, 0)
    assert st["paths"] == 4 and len(off) == 5
    fails(lambda: dev.gcode_steps_source(4), "merged")
    convert(dev, steps)


@pytest.mark.parametrize("which", ["merge", "simplify"])
def test_an_explicit_empty_list(dev, steps, which):
    convert(dev, steps)
    if which == "merge":
        out = dev.gcode_merge(*EMPTY, None, 1, False)
        assert out[5]["paths_out"] == 0 and out[0].tolist() == [0] and len(out[1]) == 0
    else:
        out = dev.gcode_simplify(*EMPTY, 0)
        assert out[3]["points_out"] == 0 and out[0].tolist() == [0] and len(out[1]) == 0
    off, pts = dev.gcode_steps_fetch(0, 0)
    assert off.tolist() == [0] and len(pts) == 0
    fails(lambda: dev.gcode_steps_source(0), "merged")                        # five were resident: the sources do not name the empty list
    assert len(dev.gcode_order(None, n=0)) == 0
    fails(lambda: dev.gcode_order(None, n=1), "orip_gcode_order:", "1 paths asked for, 0 step polylines resident")
    convert(dev, steps)
