"""The parameter sweeps of tests/test_gpu_vector_params.py deserve the name: on the sweep inputs of tests/param_cases.py every swept value changes the
oracle's result (a sweep over an input that a parameter does not touch compares nothing), the two families of values that provably cannot change it
are asserted to leave it exactly alone, and the host's derived parameter blocks equal the oracle's for every swept configuration.  CPU only."""
import numpy as np
import pytest

from oracle import oracle as O
import param_cases as C
from util import same_polys, cfgobj


def _same08(a, b):
    return a[1] == b[1] and same_polys(a[0], b[0])


def _same10(a, b, names):
    return all(a[n][1] == b[n][1] and same_polys(a[n][0], b[n][0]) for n in names)


def _same12(a, b):
    if [o["type"] for o in a] != [o["type"] for o in b]:
        return False
    return all(np.array_equal(x["points"], y["points"]) if x["type"] == "line" else (x["x"], x["y"]) == (y["x"], y["y"]) for x, y in zip(a, b))


_BASE08 = dict(O.DEFAULTS, pixels_per_mm=C.PPM08)


@pytest.fixture(scope="module")
def in08():
    polys = C.sweep_input08(*O.canvas_size(_BASE08))
    return polys, O.stage08_layer(polys, O.derived08(_BASE08))


def test_sweep_input08_is_what_it_says():
    """gaps over 20 .. 130 px, fragments with extents over 3 .. 25 px, closed shapes with perimeters over 60 .. 350 px and diameters over 5 .. 70 px"""
    polys = [np.asarray(p).reshape(-1, 2).astype(np.float64) for p in C.sweep_input08(*O.canvas_size(_BASE08))]
    gaps = np.concatenate([np.hypot(*(p[1:] - p[:-1]).T) for p in polys if len(p) > 1])
    assert all(((gaps >= lo) & (gaps < lo + 10)).any() for lo in range(20, 130, 10))
    ext = lambda p: float((p.max(0) - p.min(0)).max())
    frag = sorted(ext(p) for p in polys if len(p) > 50 and ext(p) <= 25)
    assert frag[0] <= 3 and frag[-1] == 25 and all(b - a <= 4 for a, b in zip(frag, frag[1:]))
    closed = [p for p in polys if len(p) > 3 and (p[0] == p[-1]).all() and ext(p) <= 71]
    per = sorted(float(np.hypot(*(p[1:] - p[:-1]).T).sum()) for p in closed)
    dia = sorted(ext(p) for p in closed)
    assert dia[0] <= 5 and dia[-1] >= 69 and all(b - a <= 12 for a, b in zip(dia, dia[1:]))
    assert per[0] <= 60 and per[-1] >= 350 and all(b - a <= 60 for a, b in zip(per, per[1:]))


@pytest.mark.parametrize("key,value", C.SWEEP08, ids=lambda v: str(v))
def test_stage08_swept_value_changes_the_result(in08, key, value):
    polys, base = in08
    assert not _same08(O.stage08_layer(polys, O.derived08(dict(_BASE08, **{key: value}))), base), (key, value)


@pytest.mark.parametrize("col_rad,stride", C.STRIDE_BELOW08)
def test_stage08_stride_below_radius_changes_the_result(in08, col_rad, stride):
    """against the same radius with stride = radius: what only the 3 x 3 lookup of too small cells does"""
    polys, _ = in08
    cfg = dict(_BASE08, collision_radius_intra_px=col_rad)
    at_radius = O.stage08_layer(polys, O.derived08(dict(cfg, hash_stride_px=col_rad)))
    assert not _same08(O.stage08_layer(polys, O.derived08(dict(cfg, hash_stride_px=stride))), at_radius), (col_rad, stride)


@pytest.mark.parametrize("key,value", C.STRIDE_IDENTITY08 + C.JUMP_IDENTITY08, ids=lambda v: str(v))
def test_stage08_identities(in08, key, value):
    """hash_stride_px >= radius, or 0: the default result exactly (the device's direct comparison relies on it).  max_join_jump_px: no accepted value
    changes anything (param_cases.JUMP_IDENTITY08 says why; the device has no split kernel because of it)."""
    polys, base = in08
    assert _same08(O.stage08_layer(polys, O.derived08(dict(_BASE08, **{key: value}))), base), (key, value)
    W, H = O.canvas_size(dict(O.DEFAULTS, pixels_per_mm=C.RETRACED_PPM))
    cfg = dict(O.DEFAULTS, pixels_per_mm=C.RETRACED_PPM)
    rp = C.retraced_input08(W, H)
    assert _same08(O.stage08_layer(rp, O.derived08(dict(cfg, **{key: value}))), O.stage08_layer(rp, O.derived08(cfg))), (key, value)


def test_stage08_combinations_differ_from_defaults_and_from_each_other(in08):
    polys, base = in08
    res = [O.stage08_layer(polys, O.derived08(dict(_BASE08, **c))) for c in C.combos08()]
    assert len(res) >= 6
    for i, r in enumerate(res):
        assert not _same08(r, base), i
        assert all(not _same08(r, q) for q in res[:i]), i


def test_stage08_struct_only_fields_change_the_result(in08):
    """post_on and tap_max_v have no config key; the GPU sweep sets them through the ABI struct"""
    polys, base = in08
    for kw in (dict(post_on=0), dict(tap_max_v=3), dict(tap_max_v=50)):
        d = dict(zip(_FIELDS08, O.derived08(_BASE08))); d.update(kw)
        got = O.stage08_layer(polys, np.array([d[k] for k in _FIELDS08], np.float64))
        assert _same08(got, base) == (kw == dict(tap_max_v=50)), kw


_FIELDS08 = ["tap_diam", "tap_max_dim", "min_keep", "tap_max_per", "tap_max_v", "sample_step", "tail_len_px", "col_rad", "grid_stride", "max_jump",
             "post_on", "post_brush", "post_step", "post_eps", "post_minlen", "W", "H", "brush_forbid"]
_FIELDS10 = ["tap_diam", "min_keep", "tap_max_per", "tap_max_v", "max_jump", "D_lines", "D_taps", "step_px", "W", "H"]


@pytest.mark.parametrize("which", ["random", "edge"])
def test_stage10_swept_values(which):
    over, intra = C.random_input10() if which == "random" else C.edge_input10()
    cfg = dict(O.DEFAULTS, **over)
    base = O.stage10(intra, cfg)
    for key, value in C.SWEEP10:
        assert not _same10(O.stage10(intra, dict(cfg, **{key: value})), base, C.NAMES10), (key, value)
    for key, value in C.JUMP_IDENTITY10:
        assert _same10(O.stage10(intra, dict(cfg, **{key: value})), base, C.NAMES10), (key, value)
    for D_lines, D_taps in C.STRUCT10:      # brush sizes the config cannot express (it ties both to pen_width_px)
        prm = dict(zip(_FIELDS10, O.derived10(cfg))); prm.update(D_lines=D_lines, D_taps=D_taps)
        assert not _same10(C.stage10_with(O, intra, cfg, np.array([prm[k] for k in _FIELDS10], np.float64)), base, C.NAMES10), (D_lines, D_taps)


def test_stage12_swept_values():
    lines, taps = C.input12(C.SENSITIVE12)
    base = O.stage12(lines, taps, dict(O.DEFAULTS))
    for key, value in C.SWEEP12:
        assert not _same12(O.stage12(lines, taps, dict(O.DEFAULTS, **{key: value})), base), (key, value)
    assert _same12(O.stage12(lines, taps, dict(O.DEFAULTS, pen_width_px=60)), base) and _same12(O.stage12(lines, taps, dict(O.DEFAULTS, pen_width_px=24)), base)


def _all_swept_configs():
    out = [dict(_BASE08, **{k: v}) for k, v in C.SWEEP08 + C.STRIDE_IDENTITY08 + C.JUMP_IDENTITY08]
    out += [dict(_BASE08, collision_radius_intra_px=r, hash_stride_px=s) for r, s in C.STRIDE_BELOW08]
    out += [dict(_BASE08, **c) for c in C.combos08()]
    out += [dict(O.DEFAULTS, pixels_per_mm=8, **{k: v}) for k, v in C.SWEEP10 + C.JUMP_IDENTITY10]
    out += [dict(O.DEFAULTS, pen_width_px=p) for p in C.PEN12]
    out += [dict(O.DEFAULTS, **over) for _, over, _ in C.CASES05]
    out += [dict(O.DEFAULTS, **over) for _, over, _ in C.CHAIN]
    return out


def test_host_derived_parameters_equal_the_oracles():
    """orip.stages.params08 / params10 / r_insert12 against oracle.derived08 / derived10 / max(80, pen), field by field, for every swept configuration"""
    from orip import stages as S
    cfgs = _all_swept_configs()
    assert len(cfgs) > 60
    for cfgd in cfgs:
        cfg = cfgobj(cfgd)
        p8, w8 = S.params08(cfg), O.derived08(cfgd)
        assert [n for n, _ in p8._fields_] == _FIELDS08 and len(w8) == len(_FIELDS08)
        for n, w in zip(_FIELDS08, w8):
            assert float(getattr(p8, n)) == float(w), (n, cfgd)
        p10, w10 = S.params10(cfg), O.derived10(cfgd)
        assert [n for n, _ in p10._fields_] == _FIELDS10 and len(w10) == len(_FIELDS10)
        for n, w in zip(_FIELDS10, w10):
            assert float(getattr(p10, n)) == float(w), (n, cfgd)
        assert S.r_insert12(cfg) == float(max(80.0, cfgd["pen_width_px"])), cfgd
        assert S.r_insert12(cfg) == float(max(80, cfgd["pen_width_px"]))


def test_brush_sizes_of_the_swept_radii():
    """brush_forbid = max(1, round(2 r)) and the stamp radius brush_forbid // 2: 0.4 -> 1 -> 0 (a capsule of radius 0: the pixels of the segment itself),
    25.5 -> 51 -> 25 (an odd brush loses its half pixel), 31 -> 62 -> 31"""
    got = {r: int(O.derived08(dict(O.DEFAULTS, collision_radius_intra_px=r))[_FIELDS08.index("brush_forbid")]) for r in (0.4, 3.0, 9.0, 18.0, 25.5, 31.0)}
    assert got == {0.4: 1, 3.0: 6, 9.0: 18, 18.0: 36, 25.5: 51, 31.0: 62}
    assert [b // 2 for b in got.values()] == [0, 3, 9, 18, 25, 31]


@pytest.mark.parametrize("name,over,src", C.CASES05, ids=[c[0] for c in C.CASES05])
def test_stage05_cases_are_what_they_say(name, over, src):
    from orip.config import scale_factors, canvas_size_px, margins_px
    cfgd = dict(O.DEFAULTS, **over); cfg = cfgobj(cfgd)
    assert scale_factors(cfg, *src) == O.scale_factors(src[0], src[1], cfgd)            # the host's factors are the oracle's
    assert canvas_size_px(cfg) == O.canvas_size(cfgd)
    Wc, Hc = canvas_size_px(cfg); ml, mr, mt, mb = margins_px(cfg)
    iw, ih = max(1, Wc - ml - mr), max(1, Hc - mt - mb)
    if name == "negative_margins":
        assert (ml, mr, mt) == (0, 0, 0) and mb > 0
    if name == "margins_beyond_sheet":
        assert Wc - ml - mr < 1 and Hc - mt - mb < 1
    if name == "margins_beyond_width_only":
        assert Wc - ml - mr < 1 and ih > 1
    if name.startswith("half_products"):
        ppm = cfgd["pixels_per_mm"]
        assert all((float(cfgd[k]) * ppm) % 1 == 0.5 for k in ("margin_left_mm", "margin_right_mm", "margin_top_mm", "margin_bottom_mm", "target_width_mm", "target_height_mm"))
    if name == "width_binds":
        assert iw / src[0] < ih / src[1]
    if name in ("height_binds", "one_pixel_wide"):
        assert ih / src[1] < iw / src[0]
    if name.startswith("landscape"):
        assert Wc > Hc
