"""fill_layers on the GPU: orip_fill_mask against the sequential double of tests/fill_double.py -- the segments and all six counts, by equality -- on every
named case of tests/fill_cases.py; the resident form, with the masks and a later edge detection bit for bit what they were; the consequences that need no
double; every argument check, with the context still usable; order "nearest" against tests/pens_double.py; and the stage script with stage 13 end to end.
No comparison has a tolerance."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fill_cases as FC
import fill_double as FD
import pens_double as PD
from fill_cases import FILL, STAGES, make_output, snapshot

CASES = FC.cases()
WANT = {}


def want(name):
    """the double's answer, computed once"""
    if name not in WANT:
        WANT[name] = FD.fill_mask(*FC.args(CASES[name]))
    return WANT[name]


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def equal(got, exp):
    assert got[0].dtype == np.int32 and got[0].shape == exp[0].shape and got[1] == exp[1], (got[1], exp[1])
    assert np.array_equal(got[0], exp[0]), (got[0][:8], exp[0][:8])


# ------------------------------------------------------------------ every case against the double
@pytest.mark.parametrize("name", sorted(CASES))
def test_case(dev, name):
    equal(dev.fill_mask(*FC.args(CASES[name])), want(name))


# ------------------------------------------------------------------ the resident form
def test_the_resident_form_reads_the_masks_and_writes_nothing(dev):
    rng = np.random.RandomState(11)
    masks = np.zeros((3, 48, 64), np.uint8)
    masks[0] = CASES["random_60"]["mask"]
    masks[1, 6:40, 8:50] = 255; masks[1, 16:24, 20:30] = 0
    masks[2] = (rng.rand(48, 64) < 0.3) * 255
    c = CASES["random_60"]
    rest = FC.args(c)[1:]
    dev.set_masks(masks)
    dev.detect_edges()
    edges = [dev.get_edges(l) for l in range(3)]
    dev.set_masks(masks)
    got = [dev.fill_mask(None, *rest, layer=l) for l in range(3)]
    for l in range(3):
        equal(got[l], dev.fill_mask(masks[l], *rest))
        assert np.array_equal(dev.get_mask(l), masks[l])
    equal(got[0], want("random_60"))
    dev.detect_edges()                                                                # behind the fills: what it was without them
    for l in range(3):
        assert np.array_equal(dev.get_edges(l), edges[l]) and np.array_equal(dev.get_mask(l), masks[l])


# ------------------------------------------------------------------ the consequences that need no double
@pytest.mark.parametrize("name", ["rect_hole_p0_u3", "rect_hole_p1_u4", "rect_hole_p1_u5", "random_60", "off_canvas_y", "family_cross_serpentine", "full_u2"])
def test_the_consequences_that_need_no_double(dev, name):
    c = CASES[name]
    seg, st = dev.fill_mask(*FC.args(c))
    assert st["runs"] == st["short"] + st["segments"] and st["segments"] == len(seg) and st["on"] <= st["samples"]
    P = seg.astype(np.int64).reshape(-1, 2)
    num, den, dx, dy = c["place"]
    col, row = (P[:, 0] - dx) * den // num, (P[:, 1] - dy) * den // num                # both ends are INK
    assert (P >= 0).all() and (P[:, 0] < c["W"]).all() and (P[:, 1] < c["H"]).all()
    assert (col >= 0).all() and (col < c["mask"].shape[1]).all() and (row >= 0).all() and (row < c["mask"].shape[0]).all() and (c["mask"][row, col] != 0).all()
    fams = ([c["u"]] if c["flags"] & FC.ALONG else []) + ([(-c["u"][1], c["u"][0])] if c["flags"] & FC.ACROSS else [])
    R, D, m, im, lm = FD.frame(c["u"], c["spacing"], c["inset"], c["min_len"])
    on_line = np.zeros(len(P), bool)
    for ux, uy in fams:                                                               # |n.P - k D| <= m / 2 for the nearest k of some family, the same k at both ends
        nP = -uy * P[:, 0] + ux * P[:, 1]
        k = (2 * nP + D) // (2 * D)
        ok = 2 * np.abs(nP - k * D) <= m
        on_line |= ok & np.repeat(ok.reshape(-1, 2).all(1) & (k.reshape(-1, 2)[:, 0] == k.reshape(-1, 2)[:, 1]), 2)
    assert on_line.all()
    prev = seg
    for inset in (c["inset"] + 1, c["inset"] + 4):                                    # raising the inset never adds a segment
        seg2, st2 = dev.fill_mask(*FC.args(dict(c, inset=inset)))
        assert len(seg2) <= len(prev) and st2["runs"] == st["runs"] and st2["on"] == st["on"] and st2["short"] >= st["short"]
        lo, hi = np.minimum(prev[:, :2], prev[:, 2:]), np.maximum(prev[:, :2], prev[:, 2:])
        for s in seg2:                                                                # and what is left of a segment lies within what it was
            assert ((lo <= np.minimum(s[:2], s[2:])).all(1) & (hi >= np.maximum(s[:2], s[2:])).all(1)).any()
        prev = seg2


@pytest.mark.parametrize("name", ["rect_hole_p0_u0", "run_60_70", "run_64_127", "run_last_block"])
def test_the_closed_form_at_0_degrees(dev, name):
    seg, runs, short = FC.rows_closed_form(CASES[name])
    got, st = dev.fill_mask(*FC.args(CASES[name]))
    assert np.array_equal(got, seg) and (st["runs"], st["short"], st["segments"]) == (runs, short, len(seg))


# ------------------------------------------------------------------ the argument checks
BAD = [("W", 0), ("W", (1 << 20) + 1), ("H", 0), ("H", (1 << 20) + 1), ("place", (0, 1, 0, 0)), ("place", ((1 << 20) + 1, 1, 0, 0)), ("place", (1, 0, 0, 0)),
       ("place", (1, (1 << 20) + 1, 0, 0)), ("place", (3, 1, -(1 << 20) - 1, 0)), ("place", (3, 1, 0, (1 << 20) + 1)), ("u", (0, 0)), ("u", (4097, 0)), ("u", (0, -4097)),
       ("spacing", 1), ("spacing", (1 << 15) + 1), ("inset", -1), ("inset", (1 << 15) + 1), ("min_len", 0), ("min_len", (1 << 15) + 1), ("flags", 0), ("flags", FC.SERPENTINE),
       ("flags", 8 | FC.ALONG), ("flags", -1), ("W", 1 << 40)]


def test_every_argument_check_is_an_error_and_the_context_stays_usable(dev):
    from orip.device import OripError
    good = CASES["rect_hole_p0_u3"]
    first = dev.fill_mask(*FC.args(good))
    for key, val in BAD:
        with pytest.raises(OripError):
            dev.fill_mask(*FC.args(dict(good, **{key: val})))
    with pytest.raises(OripError):                                                    # 2^26 blocks of 64 samples or more, found before any launch
        dev.fill_mask(good["mask"], 1 << 20, 1 << 20, good["place"], (4096, 0), 2, 0, 1, FC.ALONG)
    dev.set_masks(np.zeros((2, 30, 40), np.uint8))
    for layer, shape in ((2, (30, 40)), (-1, (30, 40)), (0, (30, 41))):               # a layer that is not resident; a size that is not the resident one
        dev.H, dev.W = shape
        with pytest.raises(OripError):
            dev.fill_mask(None, *FC.args(good)[1:], layer=layer)
    dev.H, dev.W = 30, 40
    seg = np.zeros((len(first[0]), 4), np.int32)                                      # the list of the last good call is still there
    from orip.device import _p
    dev._ck(dev.L.orip_fill_fetch(dev.h, _p(seg)))
    assert np.array_equal(seg, first[0])
    equal(dev.fill_mask(*FC.args(good)), first)
    equal(dev.fill_mask(*FC.args(good)), want("rect_hole_p0_u3"))


# ------------------------------------------------------------------ order "nearest"
def test_order_nearest_is_the_pen_order_of_the_segments_ends(dev):
    from orip import stages as S
    from orip.config import Config
    from orip.stream import to_steps
    cfg = Config()
    cfg.target_width_mm, cfg.target_height_mm, cfg.pixels_per_mm = 20, 15, 10
    cfg.margin_left_mm = cfg.margin_right_mm = cfg.margin_top_mm = cfg.margin_bottom_mm = 0
    cfg._raw = {"fill": {"angle_deg": 30, "order": "nearest", "layers": {"layer_dark": {}, "layer_mid": {"order": "serpentine"}}}}
    opts = S.fill_options(cfg)
    mask = np.zeros((30, 40), np.uint8); mask[5:25, 4:36] = 255; mask[10:20, 12:28] = 0
    plain, st = S.fill_segments(mask, 40, 30, cfg, opts["layer_mid"], dev)
    equal((plain, st), FD.fill_mask(mask, 200, 150, (200, 40, 0, 0), opts["layer_mid"]["u"], 10, 3, 5, opts["layer_mid"]["flags"]))
    near, st2 = S.fill_segments(mask, 40, 30, cfg, opts["layer_dark"], dev, start=(150.0, 140.0))
    ends = np.concatenate([to_steps(plain[:, :2], 200, 150), to_steps(plain[:, 2:], 200, 150)], 1)
    order, rev = PD.order_pens_numpy(ends, np.zeros(len(plain), np.int32), 1, reverse=True, start=(150, 9))
    assert st2 == st and len(plain) > 10 and rev.any() and np.array_equal(near, np.where(rev[:, None], plain[order][:, [2, 3, 0, 1]], plain[order]))
    ops = S.fill_layer(mask, 40, 30, cfg, opts["layer_dark"], dev, start=(150.0, 140.0))
    assert len(ops) == len(near) and all(o["type"] == "line" and o["points"].dtype == np.float32 and np.array_equal(o["points"].reshape(4), s) for o, s in zip(ops, near))


# ------------------------------------------------------------------ end to end: the stage script, then stage 13
def run_script(name, out, *args):
    env = dict(os.environ, CONFIG_PATH=str(out / "config.json"))
    r = subprocess.run([sys.executable, os.path.join(STAGES, name), *args], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_stage_script_then_stage_13(tmp_path):
    out, masks = make_output(tmp_path, FILL)
    outline = sum(1 for n in ("layer_dark", "layer_light") for o in pickle.loads((out / n / "ops.pkl").read_bytes()) if o["type"] == "line")
    report = [l for l in run_script("fill_layers.py", out).splitlines() if l.startswith("[fill] layer_")]
    segments = [int(l.split("segments=")[1].split()[0]) for l in report]
    assert len(segments) == 2 and min(segments) > 3
    for i, name in enumerate(("layer_dark", "layer_light")):                          # the double agrees with the report, count by count
        o = dict(u=(3547, 2048), spacing=(10, 7)[i], inset=3, min_len=5, flags=(7, 3)[i])
        st = FD.fill_mask(masks[i], 200, 150, (200, 40, 0, 0), o["u"], o["spacing"], o["inset"], o["min_len"], o["flags"])[1]
        assert all(f"{k}={st[k]}" in report[i] for k in FD.STATS), (report[i], st)
    after = snapshot(out)
    run_script("fill_layers.py", out)                                                 # a second run leaves identical files
    assert snapshot(out) == after
    run_script("13_build_stream.py", out)
    meta = json.loads((out / "plot_stream.json").read_text())
    assert meta["lines"] == outline + sum(segments) and meta["taps"] == 2


def test_without_a_fill_object_nothing_is_written_and_the_stream_is_what_it_was(tmp_path):
    a, _ = make_output(tmp_path / "a", None)
    b, _ = make_output(tmp_path / "b", None)
    before = snapshot(a)
    assert "no fill object" in run_script("fill_layers.py", a)
    assert snapshot(a) == before
    run_script("13_build_stream.py", a)
    run_script("13_build_stream.py", b)
    assert (a / "plot_stream.bin").read_bytes() == (b / "plot_stream.bin").read_bytes() and (a / "plot_stream.json").read_bytes() == (b / "plot_stream.json").read_bytes()


def test_pipeline_runs_the_fill_stage_in_front_of_step_13(tmp_path):
    out, _ = make_output(tmp_path, None)
    r = subprocess.run([sys.executable, os.path.join(STAGES, "pipeline.py"), "in.png", "--output", str(out), "--start-step", "13", "--end-step", "13", "--fill",
                        json.dumps({"layers": {"layer_dark": {"spacing_mm": 0.8}}})], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cfg = json.loads((out / "config.json").read_text())
    assert cfg["fill"] == {"layers": {"layer_dark": {"spacing_mm": 0.8}}} and cfg["pixels_per_mm"] == 10
    segs = int(r.stdout.split("[fill] layer_dark:")[1].split("segments=")[1].split()[0])
    assert r.stdout.index("[fill] layer_dark:") < r.stdout.index("[13/14]") and segs > 3
    assert json.loads((out / "plot_stream.json").read_text())["lines"] == 2 + segs and not (out / "layer_light" / "ops_filled.pkl").exists()
