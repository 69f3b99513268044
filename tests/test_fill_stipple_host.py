"""fill stipple on the host, no GPU: the double of tests/fill_stipple_double.py against what the rule implies (the pinned counts, its closed form at radius 0,
what the named cases are named for), orip.stages.fill_options with every new key and every refusal, and the stage script's file handling with the double
injected for the device.  Every comparison is equality."""
import json
import pickle
import sys

import numpy as np
import pytest

import fill_stipple_cases as SC
import fill_stipple_double as SD
import pens_double as PD

from fill_cases import FILL, STAGES, make_output, snapshot

CASES = SC.cases()
ZERO = SC.zero_radius_cases()
WANT = {}


def want(name):
    if name not in WANT:
        WANT[name] = SD.fill_stipple(*SC.args(CASES[name]))
    return WANT[name]


# ------------------------------------------------------------------ the double
def test_the_threshold_is_a_permutation_of_0_to_63():
    T = [[SD.bayer(i, j) for i in range(8)] for j in range(8)]
    assert sorted(v for row in T for v in row) == list(range(64)) and T[0] == [0, 32, 8, 40, 2, 34, 10, 42]
    assert all(SD.bayer(i + 8 * a, j + 8 * b) == T[j][i] for i in range(8) for j in range(8) for a in (1, 5) for b in (2, 3))


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_double_adds_up(name):
    c = CASES[name]
    xy, st = want(name)
    assert st["ink"] == st["near"] + st["light"] + st["dots"] and st["dots"] == len(xy) and st["ink"] <= st["candidates"]
    assert xy.dtype == np.int32 and ((xy >= 0) & (xy < [c["W"], c["H"]])).all() and len(set(map(tuple, xy.tolist()))) == len(xy)
    num, den, dx, dy = c["place"]
    col, row = (xy[:, 0].astype(np.int64) - dx) * den // num, (xy[:, 1].astype(np.int64) - dy) * den // num        # every dot is ink
    assert (c["mask"][row, col] != 0).all()
    if name in SC.PINNED:
        assert st == SC.PINNED[name]


@pytest.mark.parametrize("name", sorted(ZERO))
def test_the_double_equals_the_closed_form_at_radius_0(name):
    a, b = SD.fill_stipple(*SC.args(ZERO[name])), SD.closed_form(*SC.args(ZERO[name]))
    assert a[1] == b[1] and a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0])


def test_the_flat_series_is_periods_times_the_thresholds_below():
    for g, n in SC.FLAT.items():
        assert n == 4 * sum(1 for T in range(64) if 64 * (255 - g) > 255 * T) == want(f"flat_{g}")[1]["dots"]


def test_the_cases_exercise_what_they_are_named_for():
    xy = want("ramp")[0]
    thirds = [int(((xy[:, 0] >= a) & (xy[:, 0] < b)).sum()) for a, b in ((12, 84), (84, 156), (156, 229))]
    assert thirds[0] < thirds[1] < thirds[2]                                           # the dots rise from the light side to the dark side
    for name in ("rational", "rational_off"):
        c = CASES[name]
        assert want(name)[1]["candidates"] > want(name)[1]["ink"] > want(name)[1]["dots"] > 0
    assert CASES["rational"]["place"][2] < 0 and CASES["rational"]["place"][3] < 0
    b0, b1, b32 = (want(f"border_clear{r}")[1] for r in (0, 1, 32))
    assert b0["near"] == 0 and b0["ink"] == b1["ink"] and 0 < b1["near"] < b1["ink"] and 0 < b32["dots"] and b32["near"] > b32["ink"] // 2
    assert len({want(f"radii_tone{r}")[1]["dots"] for r in (0, 3, 4, 32)}) > 1 and all(want(f"radii_tone{r}")[1]["near"] == 0 for r in (0, 3, 4, 32))
    assert want("radii_clear4")[1]["near"] > 0 < want("radii_clear4")[1]["dots"] and want("radii_both32")[1]["dots"] > 0 < want("radii_both32")[1]["near"]
    below, at = want("lohi_below")[1], want("lohi_at")[1]
    assert below["dots"] == 0 and below["light"] > 0 and at["light"] == 0 and at["dots"] == below["light"]
    assert want("tone_none")[1] == want("tone_zero")[1] and np.array_equal(want("tone_none")[0], want("tone_zero")[0]) and want("tone_none")[1]["light"] == 0
    serp, plain = want("rows_serpentine")[0], want("rows_plain")[0]
    assert want("rows_plain")[1]["candidates"] == 150 * 12 and not np.array_equal(serp, plain)
    exp = np.concatenate([plain[plain[:, 1] == y][::-1] if (y // 3) & 1 else plain[plain[:, 1] == y] for y in sorted(set(plain[:, 1].tolist()))])
    assert np.array_equal(serp, exp) and all(len(set((plain[plain[:, 1] == y][:, 0] // 2 // 64).tolist())) == 3 for y in range(3, 36, 6))      # every reversed row has dots in all three of its blocks
    assert CASES["min_pitch"]["lattice"] == (2, 2, 1) and want("min_pitch")[1]["dots"] > 0
    assert want("empty")[1] == dict(candidates=want("empty")[1]["candidates"], ink=0, near=0, light=0, dots=0) and want("empty")[1]["candidates"] > 0
    assert want("off_ink")[1]["ink"] == 0 and (CASES["off_ink"]["mask"] != 0).any()
    assert want("single")[1] == dict(candidates=1, ink=1, near=0, light=0, dots=1) and want("single")[0].tolist() == [[0, 0]]
    assert all(want(f"random_{s}")[1]["dots"] > 50 for s in (1, 2, 3))


def test_the_case_past_the_cap_needs_a_second_pass_and_the_small_ones_do_not():
    cap, c = SC.launch_cap(), SC.past_the_cap()
    assert 4 * cap < SC.blocks(c) < 8 * cap and SC.blocks(c) < 1 << 26 and c["clear_rad"] == c["tone_rad"] == 0 and c["flags"] == SC.SERPENTINE
    assert max(SC.blocks(v) for v in CASES.values()) < 1024 < cap
    xy, st = SD.closed_form(*SC.args(c))
    assert st["candidates"] == 150 * ((c["H"] - 1) // 2 + 1) and st["ink"] > st["dots"] > 100000 and st["light"] > 100000
    assert (xy[-100:, 1] > c["H"] - 200).all()                                         # the dots reach the rows only a second pass visits


# ------------------------------------------------------------------ the config
def cfg_with(fill, **kw):
    from orip.config import Config
    cfg = Config()
    for k, v in kw.items():
        setattr(cfg, k, v)
    cfg._raw = {} if fill is None else {"fill": fill}
    return cfg


def test_fill_options_of_a_stipple_layer_every_key():
    from orip import lib, stages as S
    from orip.svg import stipple_lattice
    d = S.fill_options(cfg_with({"layers": {"layer_dark": {"mode": "stipple"}}}))["layer_dark"]                  # the defaults, at 40 pixels per mm
    assert d == dict(mode="stipple", lattice=stipple_lattice(40, "stagger"), inset=12, tone=True, lo=0, hi=255, tone_radius=20, tone_radius_stated=False,
                     flags=lib.FILL_STIPPLE_SERPENTINE, order="serpentine")
    e = S.fill_options(cfg_with({"mode": "stipple", "stipple_mm": 0.5, "layers": {"layer_dark": {"stipple_pattern": "square", "tone": False, "tone_lo": 30, "tone_hi": 200,
                                 "tone_radius_mm": 0.1, "inset_mm": 0, "serpentine": False, "order": "nearest"}, "layer_mid": {"mode": "hatch"}, "layer_light": {}}}))
    assert e["layer_dark"] == dict(mode="stipple", lattice=(20, 20, 0), inset=0, tone=False, lo=30, hi=200, tone_radius=4, tone_radius_stated=True, flags=0, order="nearest")
    assert e["layer_light"]["lattice"] == stipple_lattice(20, "stagger") and e["layer_light"]["tone_radius"] == 10 and "mode" not in e["layer_mid"]
    assert list(e) == [n for n in cfg_with(None).color_names if n in ("layer_dark", "layer_mid", "layer_light")]      # color_names order


def test_a_hatch_layers_entry_is_what_it_is_without_any_stipple_key():
    from orip import stages as S
    hatch = {"spacing_mm": 0.6, "angle_deg": 30, "direction": "cross", "connect": True}
    plain = S.fill_options(cfg_with({"layers": {"layer_dark": hatch}}))["layer_dark"]
    mixed = S.fill_options(cfg_with({"stipple_mm": 0.5, "tone_lo": 900, "stipple_pattern": "hexagon", "tone": 3,                  # read only where the mode is stipple
                                     "layers": {"layer_dark": dict(hatch, mode="hatch", tone_radius_mm=99), "layer_mid": {"mode": "stipple", "tone_lo": 1, "stipple_pattern": "square",
                                                                                                                         "tone": True}}}))
    assert mixed["layer_dark"] == plain and "mode" not in plain and mixed["layer_mid"]["mode"] == "stipple"
    assert S.FILL_DEFAULTS == {"spacing_mm": 1.0, "angle_deg": 45.0, "direction": "along", "inset_mm": 0.3, "min_run_mm": 0.5, "serpentine": True, "order": "serpentine"}


def test_inherited_hatch_keys_are_ignored_by_a_stipple_layer():
    from orip import stages as S
    glob = {"spacing_mm": 0.01, "angle_deg": float("inf"), "direction": "diagonal", "min_run_mm": 0, "connect": 3, "connect_mm": -1}      # each an error for a hatch layer
    o = S.fill_options(cfg_with(dict(glob, layers={"layer_dark": {"mode": "stipple"}})))["layer_dark"]
    assert o == S.fill_options(cfg_with({"layers": {"layer_dark": {"mode": "stipple"}}}))["layer_dark"]
    with pytest.raises(ValueError, match="diagonal"):
        S.fill_options(cfg_with(dict(glob, layers={"layer_dark": {}})))


ST = {"mode": "stipple"}


@pytest.mark.parametrize("fill, word", [
    ({"layers": {"layer_dark": {"mode": "dots"}}}, "mode"), ({"mode": 1, "layers": {"layer_dark": {}}}, "mode"),
    ({"layers": {"layer_dark": dict(ST, spacing_mm=1.0)}}, "spacing_mm"), ({"layers": {"layer_dark": dict(ST, angle_deg=45)}}, "angle_deg"),
    ({"layers": {"layer_dark": dict(ST, direction="along")}}, "direction"), ({"layers": {"layer_dark": dict(ST, min_run_mm=0.5)}}, "min_run_mm"),
    ({"layers": {"layer_dark": dict(ST, connect=False)}}, "connect"), ({"layers": {"layer_dark": dict(ST, connect_mm=2)}}, "connect_mm"),
    ({"layers": {"layer_dark": dict(ST, stipple_mm=0.01)}}, "stipple_mm"), ({"layers": {"layer_dark": dict(ST, stipple_mm=900)}}, "stipple_mm"),
    ({"layers": {"layer_dark": dict(ST, stipple_mm="1")}}, "stipple_mm"), ({"layers": {"layer_dark": dict(ST, stipple_pattern="hexagon")}}, "stipple_pattern"),
    ({"layers": {"layer_dark": dict(ST, tone=1)}}, "tone"), ({"layers": {"layer_dark": dict(ST, tone_lo=-1)}}, "tone_lo"),
    ({"layers": {"layer_dark": dict(ST, tone_lo=1.5)}}, "tone_lo"), ({"layers": {"layer_dark": dict(ST, tone_hi=256)}}, "tone_hi"),
    ({"layers": {"layer_dark": dict(ST, tone_hi=True)}}, "tone_hi"), ({"layers": {"layer_dark": dict(ST, tone_lo=200, tone_hi=200)}}, "tone_lo"),
    ({"layers": {"layer_dark": dict(ST, tone_radius_mm=-1)}}, "tone_radius_mm"), ({"layers": {"layer_dark": dict(ST, tone_radius_mm=None)}}, "tone_radius_mm"),
    ({"layers": {"layer_dark": dict(ST, inset_mm=-1)}}, "inset_mm"), ({"layers": {"layer_dark": dict(ST, serpentine=1)}}, "serpentine"),
    ({"layers": {"layer_dark": dict(ST, order="random")}}, "random"), ({"layers": {"layer_dark": dict(ST, stipple=1)}}, "stipple"),
    ({"stiple_mm": 1, "layers": {}}, "stiple_mm")])
def test_fill_options_refuses_and_names_it(fill, word):
    from orip import stages as S
    with pytest.raises(ValueError, match=word):
        S.fill_options(cfg_with(fill))


SMALL = dict(target_width_mm=20, target_height_mm=15, pixels_per_mm=10, margin_left_mm=0, margin_right_mm=0, margin_top_mm=0, margin_bottom_mm=0)


def test_the_radii_are_source_pixels_and_more_than_32_names_its_key():
    from orip import stages as S
    opt = lambda **kw: S.fill_options(cfg_with({"layers": {"layer_dark": dict(ST, **kw)}}, **SMALL))["layer_dark"]
    cfg = cfg_with(None, **SMALL)                                                      # 200 x 150 canvas: a 40 x 30 image is placed by 200 / 40, a 2000 x 1500 one by 200 / 2000
    assert S.fill_placement(cfg, 40, 30)[:2] == (200, 40) and S.fill_placement(cfg, 2000, 1500)[:2] == (200, 2000)
    assert S.fill_stipple_radii(cfg, opt(), 40, 30) == (1, 1)                          # ceil(3 * 40 / 200), floor(5 * 40 / 200)
    assert S.fill_stipple_radii(cfg, opt(inset_mm=0.6, tone_radius_mm=0.9), 40, 30) == (2, 1) and S.fill_stipple_radii(cfg, opt(inset_mm=0, tone_radius_mm=0), 40, 30) == (0, 0)
    assert S.fill_stipple_radii(cfg, opt(), 2000, 1500) == (30, 32)                    # the default tone radius, 50 source pixels, is capped
    assert S.fill_stipple_radii(cfg, opt(tone_radius_mm=0.3), 2000, 1500) == (30, 30)
    with pytest.raises(ValueError, match="tone_radius_mm"):
        S.fill_stipple_radii(cfg, opt(tone_radius_mm=0.5), 2000, 1500)                 # the same 50 pixels, stated
    with pytest.raises(ValueError, match="inset_mm"):
        S.fill_stipple_radii(cfg, opt(inset_mm=0.4), 2000, 1500)
    with pytest.raises(ValueError, match="inset_mm"):
        S.fill_dots(np.zeros((1500, 2000), np.uint8), None, 2000, 1500, cfg, opt(inset_mm=0.4), stipple_fn=SD.fill_stipple)


def test_fill_dots_passes_the_rule_its_arguments_and_orders_nearest():
    from orip import stages as S
    from orip.stream import to_steps
    cfg = cfg_with({"layers": {"layer_dark": dict(ST, stipple_mm=0.6, order="nearest"), "layer_mid": dict(ST, stipple_mm=0.6, tone=False, serpentine=False)}}, **SMALL)
    opts = S.fill_options(cfg)
    mask = np.zeros((30, 40), np.uint8); mask[5:25, 4:36] = 255; mask[10:20, 12:28] = 0
    tone = np.tile(np.linspace(0, 255, 40).astype(np.uint8), (30, 1))
    seen = []

    def spy(*a):
        seen.append(a)
        return SD.fill_stipple(*a)
    flat, st = S.fill_dots(mask, tone, 40, 30, cfg, opts["layer_mid"], stipple_fn=spy)
    assert seen[0][1] is None and seen[0][2:] == (200, 150, (200, 40, 0, 0), (6, 5, 3), 1, 0, 0, 255, 0) and st["light"] == 0 and st["dots"] == len(flat) > 20
    near, st2 = S.fill_dots(mask, tone, 40, 30, cfg, opts["layer_dark"], start=(150.0, 140.0), stipple_fn=spy, order_fn=PD.order_pens_numpy)
    assert seen[1][1] is tone and seen[1][-1] == 1
    plain = SD.fill_stipple(*seen[1])[0]
    p = to_steps(plain, 200, 150)
    order, _ = PD.order_pens_numpy(np.concatenate([p, p], 1), np.zeros(len(p), np.int32), 1, reverse=False, start=(150, 9))
    assert 10 < len(near) < len(flat) and near.dtype == np.int32 and np.array_equal(near, plain[order]) and not np.array_equal(order, np.arange(len(p)))
    ops = S.fill_dot_ops(near)
    assert ops == [{"type": "tap", "x": int(x), "y": int(y)} for x, y in near.tolist()] and all(type(o["x"]) is int and type(o["y"]) is int for o in ops)
    with pytest.raises(ValueError, match="tone of shape"):
        S.fill_dots(mask, tone[:, :-1], 40, 30, cfg, opts["layer_dark"], stipple_fn=spy)


# ------------------------------------------------------------------ the stage script
def stage_module():
    if STAGES not in sys.path:
        sys.path.insert(0, STAGES)
    import fill_layers
    return fill_layers


def double_fill(*a):
    import fill_double as FD
    return FD.fill_mask(*a)


STIPPLED = dict(FILL, layers=dict(FILL["layers"], layer_dark={"mode": "stipple", "stipple_mm": 0.4, "inset_mm": 0.1, "tone_radius_mm": 0.6}))


def gradient(out):
    """resized.png of the made output directory as a left-to-right gradient; -> the grey image the stage reads back"""
    from PIL import Image
    stage_module()                                                                    # puts the stages on the path
    import stage_io
    g = np.tile(np.linspace(20, 250, 40).astype(np.uint8), (30, 1))
    Image.fromarray(np.stack([g, g, g], 2)).save(out / "resized.png")
    return stage_io.read_gray(str(out / "resized.png"))


def test_the_stage_script_writes_taps_behind_the_outline_and_reports_them(tmp_path, capsys):
    from orip import stages as S
    from orip.config import load_config
    FL = stage_module()
    out, masks = make_output(tmp_path, STIPPLED)
    grey = gradient(out)
    assert grey.shape == (30, 40) and grey.dtype == np.uint8 and len(np.unique(grey)) > 30
    before = snapshot(out)
    cfg = load_config(str(out / "config.json"))
    assert FL.run(cfg, fill_fn=double_fill, order_fn=PD.order_pens_numpy, stipple_fn=SD.fill_stipple) == 0
    printed = capsys.readouterr().out.splitlines()
    after = snapshot(out)
    assert sorted(set(after) - set(before)) == ["layer_dark/ops_filled.pkl", "layer_light/ops_filled.pkl"]
    assert all(after[k] == before[k] for k in before if k != "vector_manifest.json")
    xy, st = SD.fill_stipple(masks[0], grey, 200, 150, (200, 40, 0, 0), (4, 3, 2), 1, 1, 0, 255, 1)
    assert st["dots"] > 20 and st["light"] > 0 and st["near"] > 0
    ops, filled = pickle.loads(before["layer_dark/ops.pkl"]), pickle.loads(after["layer_dark/ops_filled.pkl"])
    assert len(filled) == len(ops) + st["dots"]
    assert all(a["type"] == b["type"] and (np.array_equal(a["points"], b["points"]) if a["type"] == "line" else (a["x"], a["y"]) == (b["x"], b["y"])) for a, b in zip(filled, ops))
    tail = filled[len(ops):]
    assert all(o["type"] == "tap" and type(o["x"]) is int and type(o["y"]) is int and set(o) == {"type", "x", "y"} for o in tail)
    assert [[o["x"], o["y"]] for o in tail] == xy.tolist()
    man = json.loads(after["vector_manifest.json"])
    assert man["layers"][0]["file"] == "layer_dark/ops_filled.pkl" and man["layers"][0]["count_ops"] == len(filled)
    line = [l for l in printed if l.startswith("[fill-stipple] layer_dark:")]
    assert len(line) == 1 and not [l for l in printed if l.startswith("[fill] layer_dark")] and len([l for l in printed if l.startswith("[fill] layer_light:")]) == 1
    assert all(w in line[0] for w in ("pitch=4 row=3 shift=2 clear=1 tone_radius=1", "lo=0 hi=255 order=serpentine")) and all(f"{k}={st[k]}" in line[0] for k in SD.STATS)
    assert FL.run(load_config(str(out / "config.json")), fill_fn=double_fill, order_fn=PD.order_pens_numpy, stipple_fn=SD.fill_stipple) == 0      # a second run: identical files
    assert snapshot(out) == after


def test_a_config_without_mode_writes_what_it_wrote_before(tmp_path, capsys):
    from orip.config import load_config
    FL = stage_module()

    def never(*a, **k):
        raise AssertionError("no stipple call without the mode")
    a, _ = make_output(tmp_path / "a", FILL)
    b, _ = make_output(tmp_path / "b", STIPPLED)
    gradient(a); gradient(b)
    assert FL.run(load_config(str(a / "config.json")), fill_fn=double_fill, order_fn=PD.order_pens_numpy, stipple_fn=never) == 0
    assert "[fill-stipple]" not in capsys.readouterr().out
    assert FL.run(load_config(str(b / "config.json")), fill_fn=double_fill, order_fn=PD.order_pens_numpy, stipple_fn=SD.fill_stipple) == 0
    sa, sb = snapshot(a), snapshot(b)
    assert sa["layer_light/ops_filled.pkl"] == sb["layer_light/ops_filled.pkl"] and sa["layer_dark/ops_filled.pkl"] != sb["layer_dark/ops_filled.pkl"]
    import fill_double as FD                                                          # and the hatched layer_dark is the hatch of the double, as before
    from orip import stages as S
    o = S.fill_options(load_config(str(a / "config.json")))["layer_dark"]
    seg = FD.fill_mask(make_output(tmp_path / "c", None)[1][0], 200, 150, (200, 40, 0, 0), o["u"], o["spacing"], o["inset"], o["min_len"], o["flags"])[0]
    tail = pickle.loads(sa["layer_dark/ops_filled.pkl"])[2:]
    assert np.array_equal(np.array([t["points"].reshape(4) for t in tail]), seg.astype(np.float32))
    la, lb = json.loads(sa["vector_manifest.json"])["layers"], json.loads(sb["vector_manifest.json"])["layers"]
    assert la[1] == lb[1] and la[0]["file"] == lb[0]["file"]
