"""GPU parity of the vector stages 05, 08, 10, 12 AWAY from the default pen, radius and stride settings (tests/test_gpu_vector.py runs them at
the defaults only).  The kernels branch on exactly these numbers: the choice between the direct comparison and the sorted cell buckets behind
_PointHash.near, the capsule stamp radius, the tap / tiny / keep thresholds, the tail length, the brush radii of stage 10, R_insert of stage 12,
offsets and scale of stage 05.  Expected values come from the oracle, which tests/test_oracle_golden_e2e.py pins to the reference at two such settings
(golden_e2e_c / d); tests/test_oracle_params.py shows on the CPU that every swept value changes the expected result on these inputs.
Everything is equality: point lists with their order, taps, op kinds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import param_cases as C
from util import same_polys, cfgobj, compare_resident, compare_ops


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


_BASE = {"sweep": dict(O.DEFAULTS, pixels_per_mm=C.PPM08), "retraced": dict(O.DEFAULTS, pixels_per_mm=C.RETRACED_PPM)}
_INPUT = {}


def _input08(which):
    if which not in _INPUT:
        W, H = O.canvas_size(_BASE[which])
        _INPUT[which] = C.sweep_input08(W, H) if which == "sweep" else C.retraced_input08(W, H)
    return _INPUT[which]


def _check08(dev, polys, cfgd, what=None):
    from orip import stages as S
    want_l, want_t = O.stage08_layer(polys, O.derived08(cfgd))
    got_l, got_t = S.dedup_layer(polys, cfgobj(cfgd), dev)
    assert got_t == want_t, what
    assert same_polys(got_l, want_l), (what, len(got_l), len(want_l))
    return got_l, got_t


# ---------------------------------------------------------------- stage 08
@pytest.mark.parametrize("which", ["sweep", "retraced"])
@pytest.mark.parametrize("key,value", C.SWEEP08 + C.STRIDE_IDENTITY08 + C.JUMP_IDENTITY08, ids=lambda v: str(v))
def test_stage08_one_parameter(dev, monkeypatch, which, key, value):
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    _check08(dev, _input08(which), dict(_BASE[which], **{key: value}), (key, value))


@pytest.mark.parametrize("which", ["sweep", "retraced"])
@pytest.mark.parametrize("i", range(len(C.combos08())))
def test_stage08_combinations(dev, monkeypatch, which, i):
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    over = C.combos08()[i]
    _check08(dev, _input08(which), dict(_BASE[which], **over), over)


@pytest.mark.parametrize("which", ["sweep", "retraced"])
@pytest.mark.parametrize("col_rad,stride", C.STRIDE_BELOW08 + [(25.5, 18.0), (31.0, 18.0), (31.0, 30.9)])
def test_stage08_stride_below_radius(dev, monkeypatch, which, col_rad, stride):
    """With cells smaller than the radius the reference's 3 x 3 lookup misses points inside the radius: only the sorted buckets reproduce that, so the
    device must take them by itself, and ORIP_HASH_SORT (which forces them) must change nothing."""
    cfgd = dict(_BASE[which], collision_radius_intra_px=col_rad, hash_stride_px=stride)
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    got = _check08(dev, _input08(which), cfgd, (col_rad, stride))
    monkeypatch.setenv("ORIP_HASH_SORT", "1")
    forced = _check08(dev, _input08(which), cfgd, (col_rad, stride, "forced"))
    assert forced[1] == got[1] and same_polys(forced[0], got[0])


@pytest.mark.parametrize("which", ["sweep", "retraced"])
@pytest.mark.parametrize("key,value", C.STRIDE_IDENTITY08 + [("hash_stride_px", 18.0), ("collision_radius_intra_px", 9.0), ("collision_radius_intra_px", 0.4)], ids=lambda v: str(v))
def test_stage08_both_forms_of_near_at_or_above_the_radius(dev, monkeypatch, which, key, value):
    """stride >= radius: the direct comparison and the buckets are both legal and must agree (the existing hook test runs this at stride = radius = 18 only)"""
    cfgd = dict(_BASE[which], **{key: value})
    for forced in (False, True):
        if forced:
            monkeypatch.setenv("ORIP_HASH_SORT", "1")
        else:
            monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
        _check08(dev, _input08(which), cfgd, (key, value, forced))


@pytest.mark.parametrize("which", ["sweep", "retraced"])
@pytest.mark.parametrize("kw", [dict(post_on=0), dict(tap_max_v=3), dict(tap_max_v=50), dict(post_on=0, tap_max_v=3, col_rad=25.5, brush_forbid=51, grid_stride=6.0)],
                         ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_stage08_struct_only_fields(dev, monkeypatch, which, kw):
    """post_on and tap_max_v: no config key reaches them, include/orip.h exposes them"""
    from orip import lib as L, stages as S
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    polys = _input08(which)
    prm = S.params08(cfgobj(_BASE[which]))
    names = [n for n, _ in prm._fields_]
    want_prm = dict(zip(names, O.derived08(_BASE[which])))
    for k, v in kw.items():
        setattr(prm, k, v); want_prm[k] = v
    want_l, want_t = O.stage08_layer(polys, np.array([want_prm[n] for n in names], np.float64))
    dev.set_polys(L.SLOT_SORTED, 0, polys)
    dev.dedup_layer(0, prm)
    assert dev.get_taps(L.TAPS_INTRA, 0) == want_t, kw
    assert same_polys(dev.get_polys(L.SLOT_LINES_INTRA, 0), want_l), kw


@pytest.mark.parametrize("key,value", [("collision_radius_intra_px", 0.4), ("collision_radius_intra_px", 25.5), ("hash_stride_px", 4.0), ("dedup_sample_step", 3),
                                       ("ignore_tail_points_intra", 0), ("tap_max_dim", 40), ("pen_radius_px", 50)], ids=lambda v: str(v))
def test_stage08_edge_inputs_away_from_defaults(dev, monkeypatch, key, value):
    """the degenerate inputs of tests/edge_cases.py (empty, zero length, duplicates, off canvas, closed loops, a spiral, 5000 points)"""
    import edge_cases as E
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    cfgd = dict(_BASE["sweep"], **{key: value})
    for name, polys in sorted(E.cases08(*O.canvas_size(cfgd)).items()):
        _check08(dev, polys, cfgd, (name, key, value))


# ---------------------------------------------------------------- stage 10
def _same10(got, want, names, what):
    for n in names:
        assert got[n][1] == want[n][1], (what, n)
        assert same_polys(got[n][0], want[n][0]), (what, n)


def _paint(monkeypatch, paint):
    if paint == "separable":
        monkeypatch.setenv("ORIP_PAINT_SEPARABLE", "1")
    else:
        monkeypatch.delenv("ORIP_PAINT_SEPARABLE", raising=False)


@pytest.mark.parametrize("paint", ["discs", "separable"])
@pytest.mark.parametrize("which", ["random", "edge"])
@pytest.mark.parametrize("key,value", C.SWEEP10 + C.JUMP_IDENTITY10, ids=lambda v: str(v))
def test_stage10_one_parameter(dev, monkeypatch, paint, which, key, value):
    from orip import stages as S
    _paint(monkeypatch, paint)
    over, intra = C.random_input10() if which == "random" else C.edge_input10()
    cfgd = dict(O.DEFAULTS, **over); cfgd[key] = value
    _same10(S.dedup_cross(intra, cfgobj(cfgd), dev), O.stage10(intra, cfgd), C.NAMES10, (key, value))


@pytest.mark.parametrize("paint", ["discs", "separable"])
@pytest.mark.parametrize("which", ["random", "edge"])
@pytest.mark.parametrize("D_lines,D_taps", C.STRUCT10)
def test_stage10_brushes_through_the_struct(dev, monkeypatch, paint, which, D_lines, D_taps):
    """D_lines != D_taps (the config ties both to the pen), up to the largest tap radius the stage takes (D_taps 400 -> 200)"""
    from orip import lib as L, stages as S
    _paint(monkeypatch, paint)
    over, intra = C.random_input10() if which == "random" else C.edge_input10()
    cfgd = dict(O.DEFAULTS, **over)
    prm = S.params10(cfgobj(cfgd)); prm.D_lines = D_lines; prm.D_taps = D_taps
    names = [n for n, _ in prm._fields_]
    want_prm = dict(zip(names, O.derived10(cfgd))); want_prm.update(D_lines=D_lines, D_taps=D_taps)
    want = C.stage10_with(O, intra, cfgd, np.array([want_prm[n] for n in names], np.float64))
    lnames = list(cfgd["color_names"])
    for l, n in enumerate(lnames):
        dev.set_polys(L.SLOT_LINES_INTRA, l, intra[n][0]); dev.set_taps(L.TAPS_INTRA, l, intra[n][1])
    dev.dedup_cross(sorted(range(len(lnames)), key=lambda l: S.darkness_rank10(lnames[l])), prm)
    got = {n: (dev.get_polys(L.SLOT_LINES_CROSS, l), dev.get_taps(L.TAPS_CROSS, l)) for l, n in enumerate(lnames)}
    _same10(got, want, lnames, (D_lines, D_taps))


# ---------------------------------------------------------------- stage 12
def _same_ops(got, want, what):
    assert [o["type"] for o in got] == [o["type"] for o in want], what
    for a, b in zip(got, want):
        if a["type"] == "line":
            assert np.array_equal(a["points"], b["points"]), what
        else:
            assert (a["x"], a["y"]) == (b["x"], b["y"]), what


@pytest.mark.parametrize("pen", C.PEN12)
@pytest.mark.parametrize("case", C.CASES12)
def test_stage12_insert_radius(dev, pen, case):
    """R_insert = max(80, pen_width_px) = 80 / 81 / 200 / 1000"""
    from orip import stages as S
    lines, taps = C.input12(case)
    cfgd = dict(O.DEFAULTS, pen_width_px=pen)
    _same_ops(S.plot_order(lines, taps, cfgobj(cfgd), dev), O.stage12(lines, taps, cfgd), (pen, case))


# ---------------------------------------------------------------- stage 05
@pytest.mark.parametrize("name,over,src", C.CASES05, ids=[c[0] for c in C.CASES05])
def test_stage05_margins_and_sheets(dev, name, over, src):
    from orip import stages as S
    cfgd = dict(O.DEFAULTS, **over)
    for seed in range(2):
        contours = C.contours05(src[0], src[1], seed)
        assert same_polys(S.scale_vectors(contours, src[0], src[1], cfgobj(cfgd), dev), O.stage05(contours, src[0], src[1], cfgd)), (name, seed)


# ---------------------------------------------------------------- the resident chain: the parameters through orip_layer_front and the cross-layer schedule
@pytest.mark.parametrize("name,over,image", C.CHAIN, ids=[c[0] for c in C.CHAIN])
def test_resident_chain_away_from_defaults(dev, name, over, image):
    from orip import stages as S
    from orip.synth import synth_image, layer_names
    H, W, K, seed = image
    img = synth_image(H, W, K, seed=seed, sigma=5.0)
    cfgd = dict(O.DEFAULTS, color_names=layer_names(K), **over)
    want = O.run_pipeline(img, cfgd)
    assert sum(len(want["ops"][n]) for n in cfgd["color_names"]) > 20          # (the image leaves something to compare)
    ops = S.run_path(img, cfgobj(cfgd), dev)
    compare_resident(dev, cfgd, want)
    compare_ops(ops, want["ops"], cfgd["color_names"])


# ---------------------------------------------------------------- refusals
def _default08_still_right(dev):
    _check08(dev, _input08("sweep"), _BASE["sweep"], "default case after a refusal")


def _default10_still_right(dev):
    from orip import stages as S
    over, intra = C.edge_input10()
    cfgd = dict(O.DEFAULTS, **over)
    _same10(S.dedup_cross(intra, cfgobj(cfgd), dev), O.stage10(intra, cfgd), C.NAMES10, "default case after a refusal")


_LINE = [C.P([[10, 10], [200, 40], [300, 200], [90, 260], [20, 30]]), C.P([[12, 14], [205, 44], [298, 190]])]


def test_refusal_canvas_width_stage08(dev, monkeypatch):
    from orip import stages as S
    from orip.device import OripError
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    wide = dict(O.DEFAULTS, pixels_per_mm=1, target_width_mm=16384, target_height_mm=297)
    assert O.canvas_size(wide) == (16384, 297)
    with pytest.raises(OripError, match=r"canvas 16384x297 out of range"):
        S.dedup_layer(_LINE, cfgobj(wide), dev)
    _default08_still_right(dev)
    tall = dict(O.DEFAULTS, pixels_per_mm=1, target_width_mm=297, target_height_mm=16384)
    with pytest.raises(OripError, match=r"canvas 297x16384 out of range"):
        S.dedup_layer(_LINE, cfgobj(tall), dev)
    ok = dict(wide, target_width_mm=16383)
    far = _LINE + [C.P([[16000, 20], [16382, 250], [16383, 100], [16500, 90], [16100, 30]])]
    _check08(dev, far, ok, "canvas 16383 wide")
    _default08_still_right(dev)


def test_refusal_canvas_width_stage10(dev):
    from orip import stages as S
    from orip.device import OripError
    wide = dict(O.DEFAULTS, pixels_per_mm=1, target_width_mm=16384, target_height_mm=297, color_names=list(C.NAMES10))
    intra = {"layer_dark": (_LINE + [C.P([[16000, 20], [16382, 250], [16383, 100], [16500, 90]])], [(16380, 5), (40, 40)]),
             "layer_light": ([C.P([[5, 5], [250, 60], [16000, 150], [16390, 160]])], [(16382, 296), (16383, 0)])}
    with pytest.raises(OripError, match=r"canvas 16384x297 out of range"):
        S.dedup_cross(intra, cfgobj(wide), dev)
    _default10_still_right(dev)
    ok = dict(wide, target_width_mm=16383)
    _same10(S.dedup_cross(intra, cfgobj(ok), dev), O.stage10(intra, ok), C.NAMES10, "canvas 16383 wide")


def test_refusal_sample_step_against_join_jump(dev, monkeypatch):
    from orip import stages as S
    from orip.device import OripError
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    polys = _input08("sweep")
    with pytest.raises(OripError, match=r"dedup_sample_step must be < max_join_jump_px / 2"):
        S.dedup_layer(polys, cfgobj(dict(_BASE["sweep"], dedup_sample_step=40, max_join_jump_px=80.0)), dev)
    _default08_still_right(dev)
    _check08(dev, polys, dict(_BASE["sweep"], dedup_sample_step=39, max_join_jump_px=80.0), "step 39 against jump 80")


def test_refusal_join_jump_below_4_stage10(dev):
    from orip import stages as S
    from orip.device import OripError
    over, intra = C.edge_input10()
    with pytest.raises(OripError, match=r"max_join_jump_px < 4 is not supported"):
        S.dedup_cross(intra, cfgobj(dict(O.DEFAULTS, max_join_jump_px=3.9, **over)), dev)
    _default10_still_right(dev)


def test_refusal_pen_width_63_stage10(dev):
    from orip import stages as S
    from orip.device import OripError
    over, intra = C.edge_input10()
    with pytest.raises(OripError, match=r"brush radius 63/63 too large for the padded raster"):
        S.dedup_cross(intra, cfgobj(dict(O.DEFAULTS, pen_width_px=63, **over)), dev)
    _default10_still_right(dev)
    cfgd = dict(O.DEFAULTS, pen_width_px=62, **over)
    _same10(S.dedup_cross(intra, cfgobj(cfgd), dev), O.stage10(intra, cfgd), C.NAMES10, "pen 62")


def test_refusal_tap_brush_402(dev):
    from orip import lib as L, stages as S
    from orip.device import OripError
    over, intra = C.edge_input10()
    cfgd = dict(O.DEFAULTS, **over)
    prm = S.params10(cfgobj(cfgd)); prm.D_taps = 402.0
    for l, n in enumerate(cfgd["color_names"]):
        dev.set_polys(L.SLOT_LINES_INTRA, l, intra[n][0]); dev.set_taps(L.TAPS_INTRA, l, intra[n][1])
    with pytest.raises(OripError, match=r"brush radius 60/201 too large for the padded raster"):
        dev.dedup_cross(list(range(4)), prm)
    _default10_still_right(dev)
