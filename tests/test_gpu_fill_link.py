"""fill connect on the GPU: orip_fill_link against the sequential double of tests/fill_link_double.py -- off, pts and all seven counts, by equality -- on
every case of tests/fill_link_cases.py, and against its numpy form on the case that exceeds the launch cap; the resident form, with the masks and a later
edge detection bit for bit what they were; every argument check, with the context still usable, the segment list intact and orip_fill_fetch unchanged
behind a link; the fetch without a result; and the stage script with stage 13 end to end.  No comparison has a tolerance."""
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
import fill_link_cases as LC
import fill_link_double as LD
import pens_double as PD
from fill_cases import FILL, STAGES, make_output, snapshot

CASES = LC.cases()
WANT = {}


def want(name):
    """the double's answer, computed once"""
    if name not in WANT:
        WANT[name] = LD.fill_link(*LC.args(CASES[name]))
    return WANT[name]


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def equal(got, exp):
    assert got[2] == exp[2], (got[2], exp[2])
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[1].shape == exp[1].shape and np.array_equal(got[0], exp[0]), (got[0][:8], exp[0][:8])
    assert np.array_equal(got[1], exp[1]), (got[1][:8], exp[1][:8])


def fetch_segments(dev, n):
    from orip.device import _p
    seg = np.zeros((max(n, 1), 4), np.int32)
    dev._ck(dev.L.orip_fill_fetch(dev.h, _p(seg)))
    return seg[:n]


# ------------------------------------------------------------------ every case against the double
@pytest.mark.parametrize("name", sorted(CASES))
def test_case(dev, name):
    c = CASES[name]
    seg, _ = dev.fill_mask(*FC.args(c))
    equal(dev.fill_link(c["mask"], c["place"], c["reach"]), want(name))
    assert np.array_equal(fetch_segments(dev, len(seg)), seg)                         # the plain segments are still what the fill fetch returns


def test_more_pairs_than_the_waves_of_the_eligibility_kernel(dev):
    """k_fk_elig runs at most LC.ELIG_WAVES_CAP = 2048 x 4 waves, a wave a pair: here they stride"""
    c = LC.cap_pairs()
    exp = LD.fill_link_numpy(*LC.args(c))
    assert exp[2]["in_reach"] > LC.ELIG_WAVES_CAP
    dev.fill_mask(*FC.args(c))
    equal(dev.fill_link(c["mask"], c["place"], c["reach"]), exp)


# ------------------------------------------------------------------ the resident form
def test_the_resident_form_reads_the_masks_and_writes_nothing(dev):
    rng = np.random.RandomState(11)
    masks = np.zeros((3, 48, 64), np.uint8)
    masks[0] = CASES["random_60@2"]["mask"]
    masks[1, 6:40, 8:50] = 255; masks[1, 16:24, 20:30] = 0
    masks[2] = (rng.rand(48, 64) < 0.8) * 255
    c = CASES["random_60@2"]
    rest = FC.args(c)[1:]
    dev.set_masks(masks)
    dev.detect_edges()
    edges = [dev.get_edges(l) for l in range(3)]
    dev.set_masks(masks)
    for l in range(3):
        dev.fill_mask(None, *rest, layer=l)
        got = dev.fill_link(None, c["place"], c["reach"], layer=l)
        equal(dev.fill_link(masks[l], c["place"], c["reach"]), got)                   # the explicit form on the same segment list
        assert got[2]["links"] > 0 and np.array_equal(dev.get_mask(l), masks[l])
        if l == 0:
            equal(got, want("random_60@2"))
    dev.detect_edges()                                                                # behind the links: what it was without them
    for l in range(3):
        assert np.array_equal(dev.get_edges(l), edges[l]) and np.array_equal(dev.get_mask(l), masks[l])


def test_ink_is_this_calls_own_mask(dev):
    """the link reads INK from its own arguments: over a mask without the hole the refused link of hole_in_second_block is made"""
    c, whole = CASES["hole_in_second_block"], CASES["long_link"]
    dev.fill_mask(*FC.args(c))
    equal(dev.fill_link(whole["mask"], c["place"], c["reach"]), want("long_link"))
    equal(dev.fill_link(c["mask"], c["place"], c["reach"]), want("hole_in_second_block"))


# ------------------------------------------------------------------ the argument checks
BAD = [("place", (0, 1, 0, 0)), ("place", ((1 << 20) + 1, 1, 0, 0)), ("place", (1, 0, 0, 0)), ("place", (1, (1 << 20) + 1, 0, 0)), ("place", (3, 1, -(1 << 20) - 1, 0)),
       ("place", (3, 1, 0, (1 << 20) + 1)), ("reach", 0), ("reach", -1), ("reach", (1 << 15) + 1), ("reach", 1 << 40), ("mask", np.zeros((0, 4), np.uint8))]


def test_every_argument_check_is_an_error_and_everything_resident_stays(dev):
    from orip.device import OripError, _p
    good = CASES["rect_hole_p0_u3@2"]
    seg, _ = dev.fill_mask(*FC.args(good))
    first = dev.fill_link(good["mask"], good["place"], good["reach"])
    equal(first, want("rect_hole_p0_u3@2"))

    def still_there():
        off = np.zeros(first[2]["paths_out"] + 1, np.int64); pts = np.zeros((first[2]["points_out"], 2), np.int32)
        dev._ck(dev.L.orip_fill_link_fetch(dev.h, _p(off), _p(pts)))                    # the earlier link result
        assert np.array_equal(off, first[0]) and np.array_equal(pts, first[1]) and np.array_equal(fetch_segments(dev, len(seg)), seg)
    for key, val in BAD:
        a = dict(good, **{key: val})
        with pytest.raises(OripError):
            dev.fill_link(a["mask"], a["place"], a["reach"])
        still_there()
    m = np.ascontiguousarray(good["mask"])
    assert dev.L.orip_fill_link(dev.h, _p(m), 0, m.shape[0], m.shape[1], *good["place"], good["reach"], None) != 0      # NULL stats
    still_there()
    dev.set_masks(np.zeros((2, 30, 40), np.uint8))
    for layer, shape in ((2, (30, 40)), (-1, (30, 40)), (0, (30, 41))):               # a layer that is not resident; a size that is not the resident one
        dev.H, dev.W = shape
        with pytest.raises(OripError):
            dev.fill_link(None, good["place"], good["reach"], layer=layer)
    dev.H, dev.W = 30, 40
    still_there()
    with pytest.raises(OripError):                                                    # a fill that fails its own checks drops neither list
        dev.fill_mask(*FC.args(dict(FC.cases()["rect_hole_p0_u3"], spacing=1)))
    still_there()
    equal(dev.fill_link(good["mask"], good["place"], good["reach"]), first)           # the context is still usable, and the pass reads the fill's list, not its own
    equal(dev.fill_link(good["mask"], good["place"], 3 * good["spacing"]), want("rect_hole_p0_u3@3"))


def test_a_fetch_without_a_link_result_is_an_error():
    from orip.device import Device, OripError, _p
    d = Device(0)
    try:
        good = CASES["rect_hole_p0_u0@2"]
        off, pts, st = np.zeros(64, np.int64), np.zeros((64, 2), np.int32), np.zeros(7, np.int64)
        with pytest.raises(OripError):                                                # no fill to work on
            d.fill_link(good["mask"], good["place"], good["reach"])
        assert d.L.orip_fill_link_fetch(d.h, _p(off), _p(pts)) != 0                    # before any link
        seg, _ = d.fill_mask(*FC.args(good))
        assert d.L.orip_fill_link_fetch(d.h, _p(off), _p(pts)) != 0
        with pytest.raises(OripError):                                                # after a failed one
            d.fill_link(good["mask"], good["place"], 0)
        assert d.L.orip_fill_link_fetch(d.h, _p(off), _p(pts)) != 0 and "no result" in d.L.orip_last_error(d.h).decode()
        equal(d.fill_link(good["mask"], good["place"], good["reach"]), want("rect_hole_p0_u0@2"))
        d.fill_mask(*FC.args(good))                                                   # a later fill that passes its checks drops the link result
        assert d.L.orip_fill_link_fetch(d.h, _p(off), _p(pts)) != 0
        equal(d.fill_link(good["mask"], good["place"], good["reach"]), want("rect_hole_p0_u0@2"))
        e = CASES["empty@2"]                                                          # no segments: zeros and the empty list, which the fetch returns
        d.fill_mask(*FC.args(e))
        equal(d.fill_link(e["mask"], e["place"], e["reach"]), want("empty@2"))
        assert d.L.orip_fill_link(d.h, _p(e["mask"]), 0, 48, 64, *e["place"], e["reach"], _p(st)) == 0 and not st.any()
        off[0] = 7
        assert d.L.orip_fill_link_fetch(d.h, _p(off), None) == 0 and off[0] == 0
    finally:
        d.close()


# ------------------------------------------------------------------ the front door's functions
def test_fill_strokes_on_the_device(dev):
    from orip import stages as S
    from orip.config import Config
    cfg = Config()
    cfg.target_width_mm, cfg.target_height_mm, cfg.pixels_per_mm = 20, 15, 10
    cfg.margin_left_mm = cfg.margin_right_mm = cfg.margin_top_mm = cfg.margin_bottom_mm = 0
    cfg._raw = {"fill": {"angle_deg": 30, "connect": True, "layers": {"layer_dark": {"order": "nearest"}, "layer_mid": {}}}}
    opts = S.fill_options(cfg)
    mask = np.zeros((30, 40), np.uint8); mask[5:25, 4:36] = 255; mask[10:20, 12:28] = 0
    D = LD.Doubles()
    for name in ("layer_mid", "layer_dark"):
        got = S.fill_strokes(mask, 40, 30, cfg, opts[name], dev, start=(150.0, 140.0))
        exp = S.fill_strokes(mask, 40, 30, cfg, opts[name], start=(150.0, 140.0), fill_fn=D.fill, link_fn=D.link, order_fn=PD.order_pens_numpy)
        assert got[1] == exp[1] and got[2] == exp[2] and got[2]["links"] > 3 and len(got[0]) == len(exp[0]) == got[2]["paths_out"]
        assert all(a.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(got[0], exp[0]))


# ------------------------------------------------------------------ end to end: the stage script, then stage 13
def run_script(name, out, *args):
    env = dict(os.environ, CONFIG_PATH=str(out / "config.json"))
    r = subprocess.run([sys.executable, os.path.join(STAGES, name), *args], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_stage_script_then_stage_13(tmp_path):
    out, masks = make_output(tmp_path, dict(FILL, connect=True))
    outline = sum(1 for n in ("layer_dark", "layer_light") for o in pickle.loads((out / n / "ops.pkl").read_bytes()) if o["type"] == "line")
    printed = run_script("fill_layers.py", out).splitlines()
    linked = [l for l in printed if l.startswith("[fill-link] layer_")]
    assert len(linked) == 2
    paths = []
    for i, name in enumerate(("layer_dark", "layer_light")):                          # the double agrees with the report, count by count
        o = dict(u=(3547, 2048), spacing=(10, 7)[i], inset=3, min_len=5, flags=(7, 3)[i])
        st = LD.fill_link(masks[i], 200, 150, (200, 40, 0, 0), o["u"], o["spacing"], o["inset"], o["min_len"], o["flags"], 2 * o["spacing"])[2]
        assert linked[i] == f"[fill-link] {name}: reach={2 * o['spacing']} " + " ".join(f"{k}={st[k]}" for k in LD.STATS) and st["links"] > 3
        paths.append(st["paths_out"])
    run_script("13_build_stream.py", out)
    meta = json.loads((out / "plot_stream.json").read_text())
    assert meta["lines"] == outline + sum(paths) and meta["taps"] == 2


def test_the_stream_is_byte_identical_when_connect_is_absent(tmp_path):
    a, masks = make_output(tmp_path / "a", FILL)
    b, _ = make_output(tmp_path / "b", dict(FILL, connect=False, connect_mm=5))
    pa = [l.replace(str(a), "") for l in run_script("fill_layers.py", a).splitlines()]
    pb = [l.replace(str(b), "") for l in run_script("fill_layers.py", b).splitlines()]
    assert pa == pb and not any("fill-link" in l for l in pa)
    sa, sb = snapshot(a), snapshot(b)
    assert set(sa) == set(sb) and all(sa[k] == sb[k] for k in sa if k != "config.json")
    seg = [FD.fill_mask(m, 200, 150, (200, 40, 0, 0), (3547, 2048), s, 3, 5, f)[0] for m, s, f in zip(masks, (10, 7), (7, 3))]
    tail = pickle.loads(sa["layer_dark/ops_filled.pkl"])[2:]                           # the plain segments, one 2-point op each, as before
    assert len(tail) == len(seg[0]) and all(o["points"].shape == (2, 2) and np.array_equal(o["points"].reshape(4), s) for o, s in zip(tail, seg[0]))
    run_script("13_build_stream.py", a)
    run_script("13_build_stream.py", b)
    assert (a / "plot_stream.bin").read_bytes() == (b / "plot_stream.bin").read_bytes() and (a / "plot_stream.json").read_bytes() == (b / "plot_stream.json").read_bytes()
