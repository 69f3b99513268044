"""fill_layers on the host, no GPU: the double of tests/fill_double.py against what the rule implies (its own counts, the closed form at 0 degrees, the
placed runs of the named cases), orip.stages.fill_options with every refusal, the placement rational against orip.config.scale_factors, and the stage
script's file handling with the double injected for the device.  Every comparison is equality."""
import json
import os
import pickle
import sys

import numpy as np
import pytest

import fill_cases as FC
import fill_double as FD
import pens_double as PD

from fill_cases import FILL, STAGES, make_output, snapshot

CASES = FC.cases()
WANT = {}


def want(name):
    if name not in WANT:
        WANT[name] = FD.fill_mask(*FC.args(CASES[name]))
    return WANT[name]


# ------------------------------------------------------------------ the double
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_double_adds_up(name):
    c = CASES[name]
    seg, st = want(name)
    assert st["runs"] == st["short"] + st["segments"] and st["segments"] == len(seg) and st["on"] <= st["samples"] and st["runs"] <= st["on"]
    assert seg.dtype == np.int32 and ((seg[:, [0, 2]] >= 0) & (seg[:, [0, 2]] < c["W"]) & (seg[:, [1, 3]] >= 0) & (seg[:, [1, 3]] < c["H"])).all()
    for x0, y0, x1, y1 in seg.tolist():                                               # both ends are INK
        assert FD.ink(c["mask"], c["place"], x0, y0) and FD.ink(c["mask"], c["place"], x1, y1)


def test_the_cases_exercise_what_they_are_named_for():
    assert all(want(f"rect_hole_p{p}_u{d}")[1]["segments"] > 0 for p in (0, 1) for d in range(6))
    assert any(want(f"rect_hole_p{p}_u{d}")[1]["short"] > 0 for p in (0, 1) for d in range(2, 6))
    assert want("random_60")[1]["short"] > 0 and want("random_60")[1]["segments"] > 100
    for name in ("checker_x", "checker_y", "all_short"):
        st = want(name)[1]
        assert st["runs"] == st["short"] > 0 and st["segments"] == 0
    assert want("checker_x")[1]["runs"] == want("checker_x")[1]["on"]                 # every run has length 1
    assert want("empty")[1]["on"] == 0 and want("empty")[1]["samples"] > 0 and len(want("empty")[0]) == 0
    for d in (0, 1, 2, 4):                                                            # one run per line, the whole line
        st = want(f"full_u{d}")[1]
        assert st["runs"] == st["lines"] and st["on"] == st["samples"]
    assert want("run_60_70")[0].tolist()[0] == [60, 0, 70, 0]
    assert want("run_64_127")[0].tolist()[0] == [64, 0, 127, 0]
    assert want("run_last_block")[0].tolist()[0] == [194, 0, 199, 0]
    assert want("run_into_last_block")[0].tolist()[0] == [190, 0, 199, 0]
    assert want("tiny_canvas")[1] == dict(lines=1, samples=1, on=1, runs=1, short=1, segments=0)
    along, across, cross = want("family_along"), want("family_across"), want("family_cross")
    assert np.array_equal(np.concatenate([along[0], across[0]]), cross[0]) and all(along[1][k] + across[1][k] == cross[1][k] for k in FD.STATS)
    plain, serp = want("family_cross")[0], want("family_cross_serpentine")[0]
    assert not np.array_equal(plain, serp) and sorted(map(tuple, np.sort(plain.reshape(-1, 2, 2), 1).reshape(-1, 4).tolist())) == \
        sorted(map(tuple, np.sort(serp.reshape(-1, 2, 2), 1).reshape(-1, 4).tolist()))


@pytest.mark.parametrize("name", ["rect_hole_p0_u0", "run_60_70", "run_64_127", "run_last_block"])
def test_the_double_equals_the_closed_form_at_0_degrees(name):
    c = CASES[name]
    seg, runs, short = FC.rows_closed_form(c)
    got, st = want(name)
    assert np.array_equal(got, seg) and (st["runs"], st["short"]) == (runs, short)


def test_serpentine_reverses_the_odd_lines_negative_ones_included():
    c = CASES["rect_hole_p0_u2"]                                                       # serpentine, k < 0 right of the diagonal
    serp, plain = want("rect_hole_p0_u2")[0], want("negative_k_plain")[0]
    R, D, m, im, lm = FD.frame(c["u"], c["spacing"], c["inset"], c["min_len"])
    k_of = lambda s: [int(round((-c["u"][1] * x + c["u"][0] * y) / D)) for x, y in s[:, :2].tolist()]
    ks = k_of(plain)
    assert min(ks) < 0 < max(ks) and any(k & 1 for k in ks if k < 0)
    want_serp = []
    for k in sorted(set(ks)):
        rows = [s for s, kk in zip(plain.tolist(), ks) if kk == k]
        want_serp += [[x1, y1, x0, y0] for x0, y0, x1, y1 in reversed(rows)] if k & 1 else rows
    assert serp.tolist() == want_serp


# ------------------------------------------------------------------ the config
def cfg_with(fill, **kw):
    from orip.config import Config
    cfg = Config()
    for k, v in kw.items():
        setattr(cfg, k, v)
    cfg._raw = {} if fill is None else {"fill": fill}
    return cfg


def test_fill_options_defaults_and_overrides():
    from orip import lib, stages as S
    from orip.config import Config
    assert S.fill_options(Config()) is None and S.fill_options(cfg_with(None)) is None
    assert S.fill_options(cfg_with({})) == {} and S.fill_options(cfg_with({"spacing_mm": 2})) == {}      # only the named layers are filled
    o = S.fill_options(cfg_with({"spacing_mm": 1.0, "angle_deg": 45, "direction": "along", "inset_mm": 0.3, "min_run_mm": 0.5, "serpentine": True, "order": "serpentine",
                                 "layers": {"layer_mid": {"angle_deg": -45}, "layer_dark": {"spacing_mm": 0.6, "direction": "cross"}}}))
    assert list(o) == ["layer_dark", "layer_mid"]                                     # color_names order
    assert o["layer_dark"] == dict(spacing=24, inset=12, min_len=20, u=(2896, 2896), flags=lib.FILL_ALONG | lib.FILL_ACROSS | lib.FILL_SERPENTINE, order="serpentine",
                                   angle_deg=45.0)
    assert o["layer_mid"]["u"] == (2896, -2896) and o["layer_mid"]["spacing"] == 40 and o["layer_mid"]["flags"] == lib.FILL_ALONG | lib.FILL_SERPENTINE
    d = S.fill_options(cfg_with({"layers": {"layer_skin": {}}}, pixels_per_mm=10))["layer_skin"]
    assert (d["spacing"], d["inset"], d["min_len"], d["u"], d["order"]) == (10, 3, 5, (2896, 2896), "serpentine")
    e = S.fill_options(cfg_with({"serpentine": False, "direction": "across", "order": "nearest", "angle_deg": 90, "layers": {"layer_dark": {}}}))["layer_dark"]
    assert e["flags"] == lib.FILL_ACROSS and e["order"] == "nearest" and e["u"] == (0, 4096) and e["angle_deg"] == 90.0


@pytest.mark.parametrize("fill, word", [
    ({"spacing": 1.0}, "spacing"), ({"layers": {"layer_blue": {}}}, "layer_blue"), ({"layers": {"layer_dark": {"angle": 3}}}, "angle"), ({"layers": []}, "layers"),
    ({"layers": {"layer_dark": 3}}, "layer_dark"), ({"direction": "diagonal", "layers": {"layer_dark": {}}}, "diagonal"), ({"order": "random", "layers": {"layer_dark": {}}}, "random"),
    ({"serpentine": 1, "layers": {"layer_dark": {}}}, "serpentine"), ({"angle_deg": "45", "layers": {"layer_dark": {}}}, "angle_deg"),
    ({"angle_deg": float("inf"), "layers": {"layer_dark": {}}}, "angle_deg"), ({"spacing_mm": 0.01, "layers": {"layer_dark": {}}}, "spacing_mm"),
    ({"spacing_mm": 900, "layers": {"layer_dark": {}}}, "spacing_mm"), ({"inset_mm": -1, "layers": {"layer_dark": {}}}, "inset_mm"),
    ({"inset_mm": 900, "layers": {"layer_dark": {}}}, "inset_mm"), ({"min_run_mm": 0, "layers": {"layer_dark": {}}}, "min_run_mm"),
    ({"layers": {"layer_dark": {"min_run_mm": 900}}}, "min_run_mm"), ({"layers": {"layer_dark": {"spacing_mm": None}}}, "spacing_mm"), ([1], "object")])
def test_fill_options_refuses_and_names_it(fill, word):
    from orip import stages as S
    with pytest.raises(ValueError, match=word):
        S.fill_options(cfg_with(fill))


@pytest.mark.parametrize("w, h, kw", [(1414, 2000, {}), (2000, 1414, {}), (40, 30, dict(target_width_mm=20, target_height_mm=15, pixels_per_mm=10, margin_left_mm=0, margin_right_mm=0,
                                                                                      margin_top_mm=0, margin_bottom_mm=0)), (30, 40, dict(margin_left_mm=3.0, margin_top_mm=7.5)), (333, 333, {})])
def test_the_placement_is_stage_05s_scale_as_a_rational(w, h, kw):
    from fractions import Fraction
    from orip import stages as S
    from orip.config import scale_factors
    cfg = cfg_with(None, **kw)
    num, den, dx, dy = S.fill_placement(cfg, w, h)
    sx, sy, ml, mt = scale_factors(cfg, w, h)
    assert (dx, dy) == (ml, mt) and sx == sy == num / den                             # the float scale is the rational, rounded once
    from orip.config import canvas_size_px, margins_px
    (Wc, Hc), (l, r, t, b) = canvas_size_px(cfg), margins_px(cfg)
    assert Fraction(num, den) == min(Fraction(max(1, Wc - l - r), w), Fraction(max(1, Hc - t - b), h))


# ------------------------------------------------------------------ the stage script
def stage_module():
    if STAGES not in sys.path:
        sys.path.insert(0, STAGES)
    import fill_layers
    return fill_layers


def double_fill(mask, W, H, place, u, spacing, inset, min_len, flags):
    return FD.fill_mask(mask, W, H, place, u, spacing, inset, min_len, flags)


def test_the_stage_script_writes_filled_ops_and_points_the_manifest_at_them(tmp_path, capsys):
    from orip import stages as S
    from orip.config import load_config
    from orip.stream import to_steps
    FL = stage_module()
    out, masks = make_output(tmp_path, FILL)
    before = snapshot(out)
    cfg = load_config(str(out / "config.json"))
    assert FL.run(cfg, fill_fn=double_fill, order_fn=PD.order_pens_numpy) == 0
    report = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[fill] layer_")]
    after = snapshot(out)
    assert sorted(set(after) - set(before)) == ["layer_dark/ops_filled.pkl", "layer_light/ops_filled.pkl"]
    assert all(after[k] == before[k] for k in before if k != "vector_manifest.json")    # stage 12's ops.pkl among them
    man = json.loads(after["vector_manifest.json"])
    opts = S.fill_options(cfg)
    for i, name in enumerate(cfg.color_names):
        ops, filled = pickle.loads(before[f"{name}/ops.pkl"]), pickle.loads(after[f"{name}/ops_filled.pkl"])
        seg, st = FD.fill_mask(masks[i], 200, 150, (200, 40, 0, 0), opts[name]["u"], opts[name]["spacing"], opts[name]["inset"], opts[name]["min_len"], opts[name]["flags"])
        assert st["segments"] > 3
        if opts[name]["order"] == "nearest":                                          # from the end of the outline: its tap
            ends = np.concatenate([to_steps(seg[:, :2], 200, 150), to_steps(seg[:, 2:], 200, 150)], 1)
            order, rev = PD.order_pens_numpy(ends, np.zeros(len(seg), np.int32), 1, reverse=True, start=tuple(to_steps(np.array([[150, 20 + i]]), 200, 150)[0]))
            seg = np.where(rev[:, None], seg[order][:, [2, 3, 0, 1]], seg[order])
            assert rev.any() or not np.array_equal(order, np.arange(len(seg)))
        assert man["layers"][i]["file"] == f"{name}/ops_filled.pkl" and man["layers"][i]["count_ops"] == len(filled) == len(ops) + len(seg)
        assert all(a["type"] == b["type"] and (np.array_equal(a["points"], b["points"]) if a["type"] == "line" else (a["x"], a["y"]) == (b["x"], b["y"])) for a, b in zip(filled, ops))
        tail = filled[len(ops):]
        assert all(o["type"] == "line" and o["points"].dtype == np.float32 and o["points"].shape == (2, 2) for o in tail)
        assert np.array_equal(np.array([o["points"].reshape(4) for o in tail]), seg.astype(np.float32))
        assert f"angle={opts[name]['angle_deg']:.3f}" in report[i] and all(f"{k}={st[k]}" in report[i] for k in FD.STATS)
    assert FL.run(load_config(str(out / "config.json")), fill_fn=double_fill, order_fn=PD.order_pens_numpy) == 0      # a second run: identical files
    assert snapshot(out) == after


def test_the_stage_script_without_a_fill_object_writes_nothing(tmp_path, capsys):
    from orip.config import load_config
    FL = stage_module()
    out, _ = make_output(tmp_path, None)
    before = snapshot(out)

    def never(*a, **k):
        raise AssertionError("no device call without a fill object")
    assert FL.run(load_config(str(out / "config.json")), fill_fn=never, order_fn=never) == 0
    assert snapshot(out) == before and "no fill object" in capsys.readouterr().out


def test_the_stage_script_names_an_unknown_layer(tmp_path):
    from orip.config import load_config
    FL = stage_module()
    out, _ = make_output(tmp_path, {"layers": {"layer_mid": {}}})
    before = snapshot(out)
    with pytest.raises(ValueError, match="layer_mid"):
        FL.run(load_config(str(out / "config.json")), fill_fn=double_fill)
    assert snapshot(out) == before


def test_pipeline_refuses_a_fill_option_that_is_not_json(tmp_path):
    """before it writes a config or starts a stage (the merge itself is checked on the GPU, where stage 13 runs: tests/test_gpu_fill.py)"""
    import subprocess
    out = tmp_path / "o"
    r = subprocess.run([sys.executable, os.path.join(STAGES, "pipeline.py"), "in.png", "--output", str(out), "--fill", "{not json"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--fill" in r.stderr and not (out / "config.json").exists()
