"""fill stipple on the GPU: orip_fill_stipple against the sequential double of tests/fill_stipple_double.py -- the dots and all five counts, by equality -- on
every named case of tests/fill_stipple_cases.py; the resident form, with the masks and a later edge detection bit for bit what they were; the fill's segment
list, the link result and the dot list each surviving the other calls; every argument check, with the context still usable; one case past the launch cap
against the closed form; order "nearest" against tests/pens_double.py; and the stage script with stages 13 and 14 end to end.  No comparison has a
tolerance."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fill_cases as FC
import fill_stipple_cases as SC
import fill_stipple_double as SD
import pens_double as PD
from fill_cases import FILL, STAGES, make_output, snapshot

CASES = SC.cases()
WANT = {}


def want(name):
    """the double's answer, computed once"""
    if name not in WANT:
        WANT[name] = SD.fill_stipple(*SC.args(CASES[name]))
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


def fetch_dots(dev, n):
    from orip.device import _p
    xy = np.zeros((max(n, 1), 2), np.int32)
    dev._ck(dev.L.orip_fill_stipple_fetch(dev.h, _p(xy)))
    return xy[:n]


# ------------------------------------------------------------------ every case against the double
@pytest.mark.parametrize("name", sorted(CASES))
def test_case(dev, name):
    got = dev.fill_stipple(*SC.args(CASES[name]))
    equal(got, want(name))
    if name in SC.PINNED:
        assert got[1] == SC.PINNED[name]


def test_tone_none_is_a_tone_of_zero(dev):
    equal(dev.fill_stipple(*SC.args(CASES["tone_none"])), dev.fill_stipple(*SC.args(CASES["tone_zero"])))


# ------------------------------------------------------------------ the resident form
def test_the_resident_form_reads_the_masks_and_writes_nothing(dev):
    rng = np.random.RandomState(11)
    c = CASES["random_2"]
    h, w = c["mask"].shape
    masks = np.zeros((3, h, w), np.uint8)
    masks[0] = c["mask"]
    masks[1, 6:70, 8:100] = 255; masks[1, 30:40, 40:60] = 0
    masks[2] = SC.blob(h, w, 5, 0.3)
    rest = SC.args(c)[1:]
    dev.set_masks(masks)
    dev.detect_edges()
    edges = [dev.get_edges(l) for l in range(3)]
    dev.set_masks(masks)
    got = [dev.fill_stipple(None, *rest, layer=l) for l in range(3)]
    for l in range(3):
        equal(got[l], dev.fill_stipple(masks[l], *rest))
        assert np.array_equal(dev.get_mask(l), masks[l])
    equal(got[0], want("random_2"))
    assert len({g[1]["dots"] for g in got}) == 3
    dev.detect_edges()                                                                # behind the stipples: what it was without them
    for l in range(3):
        assert np.array_equal(dev.get_edges(l), edges[l]) and np.array_equal(dev.get_mask(l), masks[l])


# ------------------------------------------------------------------ three lists, none touching another
def test_the_segment_list_the_link_result_and_the_dot_list_survive_each_other(dev):
    from orip.device import _p
    f = FC.cases()["rect_hole_p0_u3"]
    seg, st = dev.fill_mask(*FC.args(f))
    off, pts, lst = dev.fill_link(f["mask"], f["place"], 20)
    assert len(seg) > 3 and lst["points_out"] == 2 * len(seg)
    dots = dev.fill_stipple(*SC.args(CASES["random_1"]))
    equal(dots, want("random_1"))
    seg2 = np.zeros_like(seg); off2 = np.zeros_like(off); pts2 = np.zeros((len(pts), 2), np.int32)
    dev._ck(dev.L.orip_fill_fetch(dev.h, _p(seg2)))
    dev._ck(dev.L.orip_fill_link_fetch(dev.h, _p(off2), _p(pts2)))
    assert np.array_equal(seg2, seg) and np.array_equal(off2, off) and np.array_equal(pts2, pts)
    off3, pts3, lst3 = dev.fill_link(f["mask"], f["place"], 20)                       # and the link still works on the fill's list
    assert lst3 == lst and np.array_equal(off3, off) and np.array_equal(pts3, pts)
    seg4, st4 = dev.fill_mask(*FC.args(f))
    dev.fill_link(f["mask"], f["place"], 20)
    assert st4 == st and np.array_equal(seg4, seg) and np.array_equal(fetch_dots(dev, len(dots[0])), dots[0])


# ------------------------------------------------------------------ the argument checks
T20 = 1 << 20
BAD = [("W", 0), ("W", T20 + 1), ("H", 0), ("H", T20 + 1), ("place", (0, 1, 0, 0)), ("place", (T20 + 1, 1, 0, 0)), ("place", (1, 0, 0, 0)), ("place", (1, T20 + 1, 0, 0)),
       ("place", (3, 1, -T20 - 1, 0)), ("place", (3, 1, 0, T20 + 1)), ("lattice", (1, 4, 0)), ("lattice", ((1 << 15) + 1, 4, 0)), ("lattice", (4, 0, 0)), ("lattice", (4, (1 << 15) + 1, 0)),
       ("lattice", (4, 4, -1)), ("lattice", (4, 4, 4)), ("clear_rad", -1), ("clear_rad", 33), ("tone_rad", -1), ("tone_rad", 33), ("lo", -1), ("hi", 256), ("lo", 255), ("hi", 0),
       ("flags", 2), ("flags", -1), ("W", 1 << 40)]


def test_every_argument_check_is_an_error_and_the_context_stays_usable(dev):
    import ctypes as C
    from orip.device import OripError, _p
    good = dict(CASES["random_3"], lo=30, hi=200)
    first = dev.fill_stipple(*SC.args(good))
    assert len(first[0]) > 50
    for key, val in BAD:
        with pytest.raises(OripError):
            dev.fill_stipple(*SC.args(dict(good, **{key: val})))
    with pytest.raises(OripError):                                                    # lo == hi
        dev.fill_stipple(*SC.args(dict(good, lo=100, hi=100)))
    with pytest.raises(OripError):                                                    # 2^26 blocks of 64 candidates or more, found before any launch
        dev.fill_stipple(good["mask"], good["tone"], T20, T20, good["place"], (2, 1, 0), 0, 0, 0, 255, 0)
    m, g = good["mask"], good["tone"]                                                  # NULL stats
    scal = [int(v) for v in (m.shape[0], m.shape[1], good["W"], good["H"], *good["place"], *good["lattice"], good["clear_rad"], good["tone_rad"], 30, 200, good["flags"])]
    assert dev.L.orip_fill_stipple(dev.h, _p(m), 0, _p(g), *scal, None) != 0
    dev.set_masks(np.zeros((2, 30, 40), np.uint8))
    for layer, shape in ((2, (30, 40)), (-1, (30, 40)), (0, (30, 41))):               # a layer that is not resident; a size that is not the resident one
        dev.H, dev.W = shape
        with pytest.raises(OripError):
            dev.fill_stipple(None, None, *SC.args(good)[2:], layer=layer)
    dev.H, dev.W = 30, 40
    assert np.array_equal(fetch_dots(dev, len(first[0])), first[0])                   # the list of the last good call is still there
    equal(dev.fill_stipple(*SC.args(good)), first)
    equal(dev.fill_stipple(*SC.args(CASES["random_3"])), want("random_3"))


def test_fetch_without_a_dot_list_is_an_error():
    from orip.device import Device, OripError
    d = Device(0)                                                                     # a context of its own: nothing has been stippled on it
    try:
        with pytest.raises(OripError):
            fetch_dots(d, 4)
        equal(d.fill_stipple(*SC.args(CASES["single"])), want("single"))
        assert fetch_dots(d, 1).tolist() == [[0, 0]]
    finally:
        d.close()


# ------------------------------------------------------------------ past the launch cap
def test_more_blocks_than_one_launch_holds(dev):
    c = SC.past_the_cap()
    assert SC.blocks(c) > 4 * SC.launch_cap()
    equal(dev.fill_stipple(*SC.args(c)), SD.closed_form(*SC.args(c)))


# ------------------------------------------------------------------ order "nearest"
def test_order_nearest_is_the_pen_order_of_the_dots(dev):
    from orip import stages as S
    from orip.config import Config
    from orip.stream import to_steps
    cfg = Config()
    cfg.target_width_mm, cfg.target_height_mm, cfg.pixels_per_mm = 20, 15, 10
    cfg.margin_left_mm = cfg.margin_right_mm = cfg.margin_top_mm = cfg.margin_bottom_mm = 0
    cfg._raw = {"fill": {"mode": "stipple", "stipple_mm": 0.6, "order": "nearest", "layers": {"layer_dark": {}, "layer_mid": {"order": "serpentine"}}}}
    opts = S.fill_options(cfg)
    mask = np.zeros((30, 40), np.uint8); mask[5:25, 4:36] = 255; mask[10:20, 12:28] = 0
    tone = np.tile(np.linspace(0, 255, 40).astype(np.uint8), (30, 1))
    plain, st = S.fill_dots(mask, tone, 40, 30, cfg, opts["layer_mid"], dev)
    equal((plain, st), SD.fill_stipple(mask, tone, 200, 150, (200, 40, 0, 0), (6, 5, 3), 1, 0, 0, 255, 1))
    near, st2 = S.fill_dots(mask, tone, 40, 30, cfg, opts["layer_dark"], dev, start=(150.0, 140.0))
    p = to_steps(plain, 200, 150)
    order, _ = PD.order_pens_numpy(np.concatenate([p, p], 1), np.zeros(len(p), np.int32), 1, reverse=False, start=(150, 9))
    assert st2 == st and len(plain) > 10 and not np.array_equal(order, np.arange(len(p))) and near.dtype == np.int32 and np.array_equal(near, plain[order])


# ------------------------------------------------------------------ end to end: the stage script, then stages 13 and 14
def run_script(name, out, *args):
    env = dict(os.environ, CONFIG_PATH=str(out / "config.json"))
    r = subprocess.run([sys.executable, os.path.join(STAGES, name), *args], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_stage_script_then_stages_13_and_14(tmp_path):
    from PIL import Image
    stippled = dict(FILL, layers=dict(FILL["layers"], layer_dark={"mode": "stipple", "stipple_mm": 0.4, "inset_mm": 0.1, "tone_radius_mm": 0.6}))
    hatched = dict(FILL, layers={"layer_light": FILL["layers"]["layer_light"]})        # the same without the stippled layer
    a, masks = make_output(tmp_path / "a", stippled)
    b, _ = make_output(tmp_path / "b", hatched)
    g = np.tile(np.linspace(20, 250, 40).astype(np.uint8), (30, 1))
    for out in (a, b):
        Image.fromarray(np.stack([g, g, g], 2)).save(out / "resized.png")
    printed = run_script("fill_layers.py", a)
    run_script("fill_layers.py", b)
    line = [l for l in printed.splitlines() if l.startswith("[fill-stipple] layer_dark:")]
    assert len(line) == 1 and "[fill] layer_dark" not in printed and "[fill] layer_light:" in printed
    xy, st = SD.fill_stipple(masks[0], g, 200, 150, (200, 40, 0, 0), (4, 3, 2), 1, 1, 0, 255, 1)
    assert st["dots"] > 20 and all(f"{k}={st[k]}" in line[0] for k in SD.STATS), (line[0], st)
    filled = pickle.loads((a / "layer_dark" / "ops_filled.pkl").read_bytes())
    assert [[o["x"], o["y"]] for o in filled[2:]] == xy.tolist() and all(o["type"] == "tap" for o in filled[2:])
    assert (a / "layer_light" / "ops_filled.pkl").read_bytes() == (b / "layer_light" / "ops_filled.pkl").read_bytes() and not (b / "layer_dark" / "ops_filled.pkl").exists()
    after = snapshot(a)
    run_script("fill_layers.py", a)                                                   # a second run leaves identical files
    assert snapshot(a) == after
    for out in (a, b):
        run_script("13_build_stream.py", out)
        run_script("14_preview_stream.py", out)
    ma, mb = json.loads((a / "plot_stream.json").read_text()), json.loads((b / "plot_stream.json").read_text())
    assert mb["taps"] == 2 and ma["taps"] == 2 + st["dots"] and ma["lines"] == mb["lines"]
    assert json.loads((a / "plot_stream_preview.json").read_text())["taps"] == 2 + st["dots"]


def test_pipeline_merges_a_stipple_layer_from_the_command_line(tmp_path):
    out, _ = make_output(tmp_path, None)
    fill = {"layers": {"layer_dark": {"mode": "stipple", "stipple_mm": 0.5, "tone": False}}}
    r = subprocess.run([sys.executable, os.path.join(STAGES, "pipeline.py"), "in.png", "--output", str(out), "--start-step", "13", "--end-step", "13", "--fill", json.dumps(fill)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert json.loads((out / "config.json").read_text())["fill"] == fill
    dots = int(r.stdout.split("[fill-stipple] layer_dark:")[1].split("dots=")[1].split()[0])
    assert r.stdout.index("[fill-stipple] layer_dark:") < r.stdout.index("[13/14]") and dots > 20
    assert json.loads((out / "plot_stream.json").read_text())["taps"] == 2 + dots
