"""Host logic of the plotter stream (orip/stream.py: the flat planner, speed plans, corner flags, byte layout, colour remap) against bytes produced by
the REFERENCE's own 13_build_stream.py / stream helper (tests/golden/golden_stream.npz, golden_stream_edges.npz, make_golden_stream.py).  CPU only: the
direction codes come from the numpy test double (tests/stream_double.py), which the first test pins to the reference's bresenham_dir_codes, the bytes from
the doubles' two packers (gcode_double.pack_numpy, stream_double.fill_bytes)."""
import json

import numpy as np
import pytest

from util import load
from stream_double import codes_numpy, fill_bytes
from gcode_double import pack_numpy

G = load("golden_stream.npz")


def _st():
    from orip import stream as ST
    return ST


def test_double_matches_reference_bresenham():
    off, codes = codes_numpy(G["bres_segs"])
    assert np.array_equal(off, G["bres_off"]) and np.array_equal(codes, G["bres_codes"])


LONG_PAIRS = [(70000, 69999), (70000, 35000), (70001, 35000), (99999, 1), (1, 99999), (131072, 65536), (131071, 3), (100000, 50000), (100000, 49999), (65537, 65536),
              (200000, 100000), (46341, 46340), (92682, 46341)]
_LONG = {}


def long_codes():
    """(segments int32 [52, 4], off, codes) of golden_stream_long.npz by the double, computed once and left unchanged"""
    if not _LONG:
        segs = load("golden_stream_long.npz")["long_segs"]
        off, codes = codes_numpy(segs)
        codes.setflags(write=False); off.setflags(write=False)
        _LONG["v"] = (segs, off, codes)
    return _LONG["v"]


def test_double_matches_reference_bresenham_on_long_segments():
    """segments of 46 341 to 200 000 steps, where 2 (k + 1) minor passes 2^31: the closed form against the sha256 of the reference's serial bresenham_dir_codes
    (tests/golden/make_golden_stream.py: write_long; the codes themselves are 5 MB)"""
    import hashlib
    L = load("golden_stream_long.npz")
    segs, off, codes = long_codes()
    # the fixture is the set it is meant to be: every pair in the four sign combinations, inside 0 .. 2^30
    d = segs[:, 2:].astype(np.int64) - segs[:, :2]
    assert [tuple(int(v) for v in r) for r in np.abs(d)[::4]] == LONG_PAIRS and len(segs) == 4 * len(LONG_PAIRS) == 52
    assert all(sorted((int(np.sign(x)), int(np.sign(y))) for x, y in d[i:i + 4]) == [(-1, -1), (-1, 1), (1, -1), (1, 1)] for i in range(0, 52, 4))
    assert (np.abs(d)[np.arange(52) // 4 * 4] == np.abs(d)).all() and segs.min() == 0 and segs.max() == 1 << 30
    assert np.array_equal(np.diff(off), L["long_steps"]) and off[-1] == 5106808
    k = np.arange(int(off[-1])) - np.repeat(off[:-1], np.diff(off))
    assert (2 * (k + 1) * np.repeat(np.abs(d).min(1), np.diff(off)) >= 1 << 31).sum() > 2_500_000          # products a 32-bit int does not hold
    for i in range(52):
        assert hashlib.sha256(codes[off[i]:off[i + 1]].tobytes()).digest() == L["long_sha256"][i].tobytes(), segs[i]


def _bytes(ST, P, sc, pack_fn=pack_numpy, initial_div=None):
    data, _, _ = ST.compile_plan(P, sc, codes_fn=codes_numpy, pack_fn=pack_fn, initial_div=initial_div)
    return np.frombuffer(data, np.uint8)


def test_travel_ramps_match_reference():
    ST = _st(); sc = ST.StreamConfig()
    for i, m in enumerate(G["travel_moves"]):
        want = G["travel_bytes"][G["travel_off"][i]:G["travel_off"][i + 1]]
        got = _bytes(ST, ST.fixed_plan([-1], [m]), sc)
        assert np.array_equal(got[:len(want)], want) and got[len(want)] == 0x3F, (i, m)


@pytest.mark.parametrize("profile", ["triangle", "scurve"])
def test_polylines_with_corners_match_reference(profile):
    """every recorded polyline as one line op through the planner, from a cursor on its first point: pen down, exactly the bytes emit_polyline
    wrote (the first of them the speed byte, as in a fresh writer), pen up, the end byte"""
    ST = _st(); sc = ST.StreamConfig(profile=profile, div_start=25, corner_div=30, corner_window_steps=800)
    off, pts = G["poly_off"], G["poly_pts"]
    for i in range(len(off) - 1):
        pl = pts[off[i]:off[i + 1]].astype(np.int64)
        want = G[f"poly_{profile}_bytes"][G[f"poly_{profile}_off"][i]:G[f"poly_{profile}_off"][i + 1]]
        P = ST.plan_ops([0, len(pl)], pl, [False], pl[0], [], False, sc)
        assert len(P.moves) == len(pl) - 1 and not P.is_travel.any()
        got = _bytes(ST, P, sc)
        assert got[0] == ST.PEN_DOWN and np.array_equal(got[1:1 + len(want)], want) and got[1 + len(want)] == ST.PEN_UP and got[2 + len(want)] == 0x3F, (profile, i)


def _layers_from(E):
    cfg = json.loads(bytes(E["cfg_json"]).decode()); man = json.loads(bytes(E["manifest_json"]).decode())
    layers = []
    for L in man["layers"]:
        n = L.get("color_name", L.get("name"))
        kinds, off, pts = E[f"ops_kinds_{n}"], E[f"ops_{n}_off"], E[f"ops_{n}_pts"]
        ops = [{"type": "line", "points": pts[off[i]:off[i + 1]].astype(np.float32)} if k == 0 else {"type": "tap", "x": int(pts[off[i], 0]), "y": int(pts[off[i], 1])}
               for i, k in enumerate(kinds)]
        layers.append((str(n), int(L.get("color_index", 0)), ops))
    return cfg, layers


def _layers_from_e2e(tag):
    return _layers_from(load(f"golden_e2e_{tag}.npz"))


def _pipeline_config(cfgd):
    from orip.config import Config
    cfg = Config()
    for k, v in cfgd.items():
        if k in Config.__dataclass_fields__:
            setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("pack_fn", [pack_numpy, fill_bytes])
@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("variant", ["", "_remap", "_env"])
def test_whole_stream_matches_reference(tag, variant, pack_fn, monkeypatch):
    ST = _st()
    from orip.config import canvas_size_px
    cfgd, layers = _layers_from_e2e(tag)
    extra = json.loads(bytes(G[f"e2e_{tag}{variant}_cfg"]).decode())
    cfg = _pipeline_config({**cfgd, **extra})
    if variant == "_env":
        monkeypatch.setenv("STREAM_FORCE_COLOR_INDEX", "6")
    W, H = canvas_size_px(cfg)
    data, meta = ST.build_stream(layers, W, H, ST.stream_config_from_pipeline(cfg), codes_fn=codes_numpy, pack_fn=pack_fn, color_maps=ST.load_color_maps(cfg))
    want = bytes(G[f"e2e_{tag}{variant}_bin"])
    assert data == want
    wj = json.loads(bytes(G[f"e2e_{tag}{variant}_json"]).decode())
    assert meta["lines"] == wj["lines"] and meta["taps"] == wj["taps"] and meta["bytes"] == wj["bytes"] and wj["target_steps"] == {"width": W, "height": H}
    assert len(data) % 1024 == 0


def edge_plot():
    """the hand-written plot of golden_stream_edges.npz (make_golden_stream.py: edge_layers): (layers, W, H, stream config, colour maps, bytes, counts)"""
    ST = _st()
    from orip.config import canvas_size_px
    E = load("golden_stream_edges.npz")
    cfgd, layers = _layers_from(E)
    cfg = _pipeline_config(cfgd)
    W, H = canvas_size_px(cfg)
    return layers, W, H, ST.stream_config_from_pipeline(cfg), ST.load_color_maps(cfg), bytes(E["bin"]), json.loads(bytes(E["json"]).decode())


@pytest.mark.parametrize("pack_fn", [pack_numpy, fill_bytes])
def test_edge_plot_matches_reference(pack_fn):
    """an empty layer, an approach to a one-point line that is then skipped, taps with and without a travel, a line that starts on the cursor, a
    repeated point, half-integer rounding, clamping that merges points, a one-step travel, a colour byte with no approach: 21 moves"""
    ST = _st()
    layers, W, H, sc, maps, want, wj = edge_plot()
    data, meta = ST.build_stream(layers, W, H, sc, codes_fn=codes_numpy, pack_fn=pack_fn, color_maps=maps)
    assert data == want
    assert meta == {"lines": wj["lines"], "taps": wj["taps"], "bytes": wj["bytes"]} and wj["target_steps"] == {"width": W, "height": H}
    assert (meta["lines"], meta["taps"], len(data)) == (9, 5, 4096)
