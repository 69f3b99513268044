"""13_build_stream on the GPU path: the HIP kernel behind orip_stream_codes against the reference's bresenham_dir_codes, the whole stream with
device codes against the reference's plot_stream.bin (tests/golden/golden_stream.npz), and the drop-in stage script on disk."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from util import load
from stream_double import codes_numpy
from test_stream_host import _layers_from_e2e, _pipeline_config, edge_plot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = load("golden_stream.npz")


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def test_direction_codes_match_reference(dev):
    off, codes = dev.stream_codes(G["bres_segs"])
    assert np.array_equal(off, G["bres_off"]) and np.array_equal(codes, G["bres_codes"])
    off, codes = dev.stream_codes(np.zeros((0, 4), np.int32))                      # no moves at all
    assert len(off) == 1 and off[0] == 0 and len(codes) == 0
    off, codes = dev.stream_codes(np.array([[3, 3, 3, 3], [3, 3, 3, 3]], np.int32))  # moves without steps
    assert np.array_equal(off, [0, 0, 0]) and len(codes) == 0


def test_direction_codes_large_random_vs_closed_form(dev):
    """a plot-sized batch (1.5 M steps): long travels, unit segments, every octant; end points reached by replaying the codes"""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 12000, (400, 4)); b = np.cumsum(rng.integers(-1, 2, (60000, 2)), axis=0) + 6000
    moves = np.concatenate([a, np.concatenate([b[:-1], b[1:]], 1)]).astype(np.int32)
    off, codes = dev.stream_codes(moves)
    o2, c2 = codes_numpy(moves)
    assert np.array_equal(off, o2) and np.array_equal(codes, c2)
    DX = np.array([0, 1, 1, 1, 0, -1, -1, -1]); DY = np.array([1, 1, 0, -1, -1, -1, 0, 1])
    ex = np.add.reduceat(DX[codes], off[:-1][np.diff(off) > 0]); ey = np.add.reduceat(DY[codes], off[:-1][np.diff(off) > 0])
    nz = np.diff(off) > 0
    assert np.array_equal(ex, (moves[:, 2] - moves[:, 0])[nz]) and np.array_equal(ey, (moves[:, 3] - moves[:, 1])[nz])


def _replayed_ends(moves, off, codes):
    """(dx, dy) reached by replaying each move's codes, for the moves that have steps"""
    DX = np.array([0, 1, 1, 1, 0, -1, -1, -1]); DY = np.array([1, 1, 0, -1, -1, -1, 0, 1])
    nz = np.diff(off) > 0
    return nz, np.add.reduceat(DX[codes], off[:-1][nz]), np.add.reduceat(DY[codes], off[:-1][nz])


def test_direction_codes_long_segments(dev):
    """golden_stream_long.npz: 52 segments of 46 341 to 200 000 steps in 0 .. 2^30, 2 (k + 1) minor at or past 2^31 on more than half of the 5.1 M steps, exact ties
    of the error term.  The double is pinned to the reference on these by test_stream_host.py; the kernel equals the double, and the codes lead to the end points"""
    from test_stream_host import long_codes
    segs, o2, c2 = long_codes()
    off, codes = dev.stream_codes(segs)
    assert np.array_equal(off, o2) and np.array_equal(codes, c2)
    nz, ex, ey = _replayed_ends(segs, off, codes)
    m = segs.astype(np.int64)
    assert nz.all() and np.array_equal(ex, m[:, 2] - m[:, 0]) and np.array_equal(ey, m[:, 3] - m[:, 1])


def _edge_batches():
    Z = [7, 7, 7, 7]                                                                          # a move without steps
    b = {}
    for total in (255, 256, 257, 512):                                                        # the last block's `t >= total` guard, one move and three
        b["one_%d" % total] = [[0, 0, total, 3]]
        b["three_%d" % total] = [[4, 9, 104, 2], [104, 2, 104, 2 + total - 150], [104, 2, 54, 40]]
    b["one_step"] = [[3, 3, 3, 4]]
    long_a, long_b, long_c = [0, 0, 900, 301], [900, 301, 13, 1200], [13, 1200, 640, 0]
    b["zero_runs"] = [Z] + [long_a] + [Z] + [long_b] + [Z, Z] + [long_c] + [Z] * 300 + [long_a] + [Z]      # first and last without steps; runs of 1, 2 and 300 in between
    return {k: np.array(v, np.int64) for k, v in b.items()}


@pytest.mark.parametrize("anchor", [0, -(1 << 31), (1 << 31) - 1 - 100000], ids=["origin", "int32_min", "int32_max_less_100000"])
def test_direction_codes_search_and_launch_edges(dev, anchor):
    """totals of 255, 256, 257 and 512 steps, n = 1, moves without steps in front, at the end and in runs of 1, 2 and 300 between long ones (the search must land on
    the last off[i] <= t), and all of it again at the two ends of int32: only the position is extreme there, so the codes are those at the origin"""
    for name, base in _edge_batches().items():
        moves = (base + anchor).astype(np.int32)
        assert np.array_equal(moves.astype(np.int64) - anchor, base)                          # inside int32
        o2, c2 = codes_numpy(base)
        if name[-3:].isdigit():
            assert int(o2[-1]) == int(name[-3:])                                              # the total the batch is named after
        off, codes = dev.stream_codes(moves)
        assert np.array_equal(off, o2) and np.array_equal(codes, c2), name
        nz, ex, ey = _replayed_ends(base, off, codes)
        assert np.array_equal(ex, (base[:, 2] - base[:, 0])[nz]) and np.array_equal(ey, (base[:, 3] - base[:, 1])[nz]), name


@pytest.mark.parametrize("tag", ["a", "b"])
def test_whole_stream_on_device_matches_reference(dev, tag):
    """direction codes and packing both on the device"""
    from orip import stream as ST
    from orip.config import canvas_size_px
    cfgd, layers = _layers_from_e2e(tag)
    cfg = _pipeline_config(cfgd)
    W, H = canvas_size_px(cfg)
    data, _ = ST.build_stream(layers, W, H, ST.stream_config_from_pipeline(cfg), color_maps=ST.load_color_maps(cfg), device=dev)
    assert data == bytes(G[f"e2e_{tag}_bin"])


def test_edge_plot_on_device_matches_reference(dev):
    """the 21 moves of golden_stream_edges.npz (test_stream_host.py: edge_plot): every branch of the planner, codes and packing on the device"""
    from orip import stream as ST
    layers, W, H, sc, maps, want, wj = edge_plot()
    data, meta = ST.build_stream(layers, W, H, sc, color_maps=maps, device=dev)
    assert data == want and meta == {"lines": wj["lines"], "taps": wj["taps"], "bytes": wj["bytes"]}


def test_stage_script_13_on_disk(tmp_path):
    """the drop-in script: vector_manifest.json + ops.pkl files in, plot_stream.bin / .json out (13:231-281), byte for byte the reference's"""
    tag = "b"
    cfgd, layers = _layers_from_e2e(tag)
    E = load(f"golden_e2e_{tag}.npz")
    out = tmp_path / "out"; out.mkdir()
    full = dict(cfgd); full["output_dir"] = str(out)
    (out / "config.json").write_text(json.dumps(full))
    for name, _, ops in layers:
        (out / name).mkdir()
        with open(out / name / "ops.pkl", "wb") as f:
            pickle.dump(ops, f)
    (out / "vector_manifest.json").write_text(bytes(E["manifest_json"]).decode())
    env = dict(os.environ, CONFIG_PATH=str(out / "config.json"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "omnirevolve-image-processor_amd", "stages", "13_build_stream.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (out / "plot_stream.bin").read_bytes() == bytes(G[f"e2e_{tag}_bin"])
    assert json.loads((out / "plot_stream.json").read_text()) == json.loads(bytes(G[f"e2e_{tag}_json"]).decode())
