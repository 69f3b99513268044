"""The resident step polylines between the calls that write them (csrc/orip_ctx.h states the contract): what orip_gcode_to_steps, orip_gcode_to_steps_clip,
orip_gcode_merge and orip_gcode_simplify leave behind after a bad argument, after an explicit upload and after n == 0, and when the sources still name
the polylines.  The drawing is the one of test_gpu_simplify.py's resident form: six paths in mm that become five polylines of fourteen points.  The last
test chains the three cutting passes (dash, occlusion, dedup; csrc/gc_cut.h) on a drawing of its own.  Every comparison is exact."""
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


CHAIN = [[(10, 10), (30, 10), (30, 30), (10, 30), (10, 10)], [(30, 10), (50, 10), (50, 30), (30, 30), (30, 10)], [(50, 50), (50, 50.2)], [(5, 60), (45, 60), (25, 60)],
         [(0, 10), (60, 10)], [(0, 40), (60, 40)], [(12, 30), (28, 30)], [(20, 50), (20, 70)]]


def test_the_cutting_passes_chained_keep_their_own_records(dev):
    """dash, occlusion and dedup one after the other on the resident list: each result, its stats and its origin are the sequential definition's
    (tests/dash_double.py, occlude_double.py, dedup_double.py applied in turn), the sources follow the composed origin, and after all three calls every
    pass's own fetch still gives that pass's origin: the three result records are independent"""
    import ctypes as C
    import dash_double as DS
    import dedup_double as DD
    import occlude_double as OD
    off_mm = np.concatenate([[0], np.cumsum([len(p) for p in CHAIN])]).astype(np.int64)
    off, pts = dev.gcode_to_steps(off_mm, np.asarray([q for p in CHAIN for q in p], np.float64), MAP)
    src = dev.gcode_steps_source(len(off) - 1)
    assert len(off) - 1 == 7 and src.tolist() == [0, 1, 3, 4, 5, 6, 7]         # the third path rounds to one point: the sources are not the identity
    pattern = np.where(pts[off[:-1], 1] == 40, 0, -1).astype(np.int32)         # the y = 40 line only
    assert pattern.tolist() == [-1, -1, -1, -1, 0, -1, -1]
    dash_args = (pattern, np.zeros(7, np.int64), np.array([0, 2], np.int32), np.array([20 * 256, 10 * 256], np.int64))
    ring = (np.array([0, 5], np.int64), np.array([(40, 0), (70, 0), (70, 20), (40, 20), (40, 0)], np.int32), np.array([1], np.int32))

    w_ds = DS.dash_numpy(off, pts, *dash_args)
    w_oc = OD.occlude_numpy(w_ds[0], w_ds[1], np.zeros(8, np.int32), *ring)
    w_dd = DD.dedup_numpy(w_oc[0], w_oc[1], None, 1)
    assert [len(w[0]) - 1 for w in (w_ds, w_oc, w_dd)] == [8, 9, 8]
    assert w_ds[2].tolist() == [0, 1, 2, 3, 4, 4, 5, 6] and w_oc[2].tolist() == [0, 1, 1, 2, 3, 4, 5, 6, 7] and w_dd[2].tolist() == [0, 1, 2, 3, 4, 5, 6, 8]
    composed = w_ds[2][w_oc[2][w_dd[2]]]
    assert composed.tolist() == [0, 1, 1, 2, 3, 4, 4, 6]

    g_ds = dev.gcode_dash(None, None, *dash_args, n=7)
    g_oc = dev.gcode_occlude(None, None, np.zeros(8, np.int32), *ring, n=8)
    g_dd = dev.gcode_dedup(None, None, None, 1, n=9)
    for got, want in ((g_ds, w_ds), (g_oc, w_oc), (g_dd, w_dd)):
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]
    assert dev.gcode_steps_source(8).tolist() == src[composed].tolist() == [0, 1, 1, 3, 4, 5, 5, 7]
    for fetch, want in ((dev.L.orip_gcode_dash_fetch, w_ds), (dev.L.orip_gcode_occlude_fetch, w_oc), (dev.L.orip_gcode_dedup_fetch, w_dd)):
        origin = np.full(len(want[2]), -1, np.int32)
        dev._ck(fetch(dev.h, origin.ctypes.data_as(C.c_void_p)))
        assert origin.tolist() == want[2].tolist()
