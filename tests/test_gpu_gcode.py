"""gcode2stream on the GPU: each kernel of csrc/gcode.hip, csrc/gcode_order.hip and the pack of csrc/stream.hip against the reference's recorded output (tests/golden/golden_gcode.npz), bit for bit; the packed
bytes against the doubles' two numpy packers on stage 13's plots; the whole tool, in process and as the script on disk, against the files the reference's main()
wrote; every degenerate input of the order; one order beyond what the reference can run, checked pair by pair against the definition; and a round trip
through the stream preview.  No comparison has a tolerance and no recorded case is left out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from util import load
import gcode_double as D
from test_gcode_host import G, MAIN_CASES, ORDER_NAMES, CONV_SETS, conv_map, options_for
from stream_double import fill_bytes
from test_stream_host import _layers_from_e2e, _pipeline_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream", "gcode2stream.py")
GS = load("golden_stream.npz")


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


# ------------------------------------------------------------------ paths to steps
@pytest.mark.parametrize("i", range(len(CONV_SETS)))
def test_to_steps_matches_reference(dev, i):
    off, pts = dev.gcode_to_steps(G["conv_off"], G["conv_pts"], conv_map(CONV_SETS[i]))
    assert np.array_equal(off, G[f"conv_{i}_off"]) and np.array_equal(pts, G[f"conv_{i}_out"])


@pytest.mark.parametrize("i", [0, 1])
def test_to_steps_exact_halves(dev, i):
    off, pts = dev.gcode_to_steps(G["conv_half_off"], G["conv_half_pts"], conv_map([2.0, bool(i), 400, 300, 0.0, 0.0, 1.0, 1.0]))
    assert np.array_equal(off, G[f"conv_half_{i}_off"]) and np.array_equal(pts, G[f"conv_half_{i}_out"])


def test_to_steps_edges(dev):
    from orip.device import OripError
    m = conv_map(CONV_SETS[0])
    off, pts = dev.gcode_to_steps(np.zeros(1, np.int64), np.zeros((0, 2)), m)                       # no paths
    assert np.array_equal(off, [0]) and len(pts) == 0
    off, pts = dev.gcode_to_steps(np.array([0, 0, 1, 1, 3, 3]), np.array([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]]), m)      # empty and one-point paths among the rest
    assert np.array_equal(off, [0, 2]) and pts.tolist() == [[20, 20], [30, 30]]
    with pytest.raises(OripError):                                                                  # int(round(inf)) raises in the reference
        dev.gcode_to_steps(np.array([0, 2]), np.array([[0.0, 0.0], [np.inf, 1.0]]), m)
    with pytest.raises(OripError):
        dev.gcode_to_steps(np.array([0, 2]), np.array([[0.0, 0.0], [1e308, 1.0]]), m)                # overflows in the multiplication
    with pytest.raises(OripError):
        dev.gcode_to_steps(np.array([0, 3]), np.array([[0.0, 0.0], [1.0, np.nan], [2.0, 2.0]]), m)
    off, pts = dev.gcode_to_steps(np.array([0, 2, 3]), np.array([[0.0, 0.0], [5.0, 1.0], [np.nan, 0.0]]), m)   # a lone point is never converted
    assert np.array_equal(off, [0, 2]) and pts.tolist() == [[0, 0], [50, 10]]
    for W, H in (((1 << 30) + 1, 10), (10, 0)):                                                     # our limit: int32 coordinates
        with pytest.raises(OripError):
            dev.gcode_to_steps(np.array([0, 2]), np.array([[0.0, 0.0], [1.0, 1.0]]), dict(m, W=W, H=H))
    big = dict(m, W=1 << 30, H=1 << 30, steps_per_mm=1e6)
    off, pts = dev.gcode_to_steps(np.array([0, 2]), np.array([[0.0, 0.0], [5000.0, 1e300]]), big)    # finite but huge: clamps
    assert pts.tolist() == [[0, 0], [(1 << 30) - 1, (1 << 30) - 1]]


def test_to_steps_large_against_double(dev):
    rng = np.random.default_rng(11)
    n = 40000
    lens = rng.integers(0, 9, n)
    off = np.concatenate([[0], np.cumsum(lens)])
    pts = np.repeat(rng.uniform(-20, 230, (n, 2)), lens, axis=0) + rng.normal(0, 0.06, (int(off[-1]), 2))       # 0.6 steps of jitter: many repeated positions
    for s in CONV_SETS[:3]:
        a = dev.gcode_to_steps(off, pts, conv_map(s)); b = D.to_steps_numpy(off, pts, conv_map(s))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(b[0]) > 100


# ------------------------------------------------------------------ order
@pytest.mark.parametrize("name", ORDER_NAMES)
def test_order_matches_reference(dev, name):
    assert np.array_equal(dev.gcode_order(G[f"order_{name}_ends"]), G[f"order_{name}_perm"])


def test_order_degenerate_inputs(dev):
    """what breaks a grid: nothing at all, one or two paths, every first point equal (ties by index alone, thousands of them), one row, one column,
    first points at the far corner of the coordinate range, a cursor that leaves the first points' box at every step"""
    from orip.device import OripError
    rng = np.random.default_rng(21)
    assert len(dev.gcode_order(np.zeros((0, 4), np.int32))) == 0
    cases = {"one": np.array([[7, 7, 1, 1]]), "two_same": np.array([[4, 4, 9, 9], [4, 4, 0, 0]]),
             "star": np.concatenate([np.full((6000, 2), 123456), rng.integers(0, 1 << 20, (6000, 2))], 1),
             "star_at_origin": np.concatenate([np.zeros((3000, 2), np.int64), rng.integers(0, 50, (3000, 2))], 1),
             "row": np.stack([rng.integers(0, 1 << 20, 4000), np.full(4000, 9), rng.integers(0, 1 << 20, 4000), rng.integers(0, 1 << 20, 4000)], 1),
             "column_dups": np.stack([np.full(4000, 1 << 30), rng.integers(0, 300, 4000), rng.integers(0, 1 << 30, 4000), rng.integers(0, 300, 4000)], 1),
             "corner": np.concatenate([(1 << 30) - rng.integers(0, 40, (2000, 2)), rng.integers(0, 1 << 30, (2000, 2))], 1),
             "two_clusters_far_apart": np.concatenate([np.concatenate([rng.integers(0, 30, (1500, 2)), (1 << 30) - rng.integers(0, 30, (1500, 2))]),
                                                       np.concatenate([(1 << 30) - rng.integers(0, 30, (1500, 2)), rng.integers(0, 30, (1500, 2))])], 1),
             "sparse_ends_outside": np.concatenate([rng.integers(5000, 6000, (3000, 2)), rng.integers(0, 12000, (3000, 2))], 1)}
    for name, e in cases.items():
        got = dev.gcode_order(e)
        assert np.array_equal(got, D.order_numpy(e)), name
    with pytest.raises(OripError):
        dev.gcode_order(np.array([[0, 0, -1, 0]]))
    with pytest.raises(OripError):
        dev.gcode_order(np.array([[0, 0, (1 << 30) + 1, 0]]))


def _shared_walk_cases():
    rng = np.random.default_rng(22)
    far = lambda k: rng.integers(0, 1 << 20, (k, 2))
    same = lambda k: np.concatenate([np.full((k, 2), 77), far(k)], 1)
    cluster = np.concatenate([1000 + rng.integers(0, 40, (300, 2)), rng.integers(0, 1 << 29, (300, 2))], 1)      # the cursor lands anywhere in the box
    return {"same_64": same(64), "same_65": same(65), "same_3000": same(3000),                                     # the two sides of GC_BIG, and far beyond
            "row_500": np.concatenate([np.stack([rng.integers(0, 1 << 20, 500), np.full(500, 9)], 1), far(500)], 1),
            "column_500_at_top": np.concatenate([np.stack([np.full(500, 1 << 30), rng.integers(0, 1 << 20, 500)], 1), far(500)], 1),
            "cluster_and_one_far": np.concatenate([cluster, [[1000 + (1 << 29), 1000 + (1 << 29), 5, 5]]]),
            "one_far": np.array([[1 << 30, 0, 3, 3]]), "two_apart": np.array([[900, 5, 0, 1 << 30], [3, 800, 7, 7]])}


@pytest.mark.parametrize("name", list(_shared_walk_cases()))
def test_order_shared_walk_shapes(dev, name):
    """orip_gcode_order through the grouped setup kernels and the shared search: a cell of exactly GC_BIG entries and of one more (four lanes against the
    whole wave), thousands on one point, one row with the cursor starting off it, one column on the last coordinate, a tight cluster with one path 2^29
    steps away (the window grows ring by ring until it meets the grid's edge on all four sides), one path and two"""
    e = _shared_walk_cases()[name]
    assert np.array_equal(dev.gcode_order(e), D.order_numpy(e))


def test_order_of_resident_polylines(dev):
    """ends = NULL: the order of the step polylines orip_gcode_to_steps left on the device"""
    from orip.device import OripError
    off, pts = dev.gcode_to_steps(G["conv_off"], G["conv_pts"], conv_map(CONV_SETS[3]))
    n = len(off) - 1
    ends = np.concatenate([pts[off[:-1]], pts[off[1:] - 1]], 1)
    got = dev.gcode_order(None, n)
    assert n > 100 and np.array_equal(got, D.order_numpy(ends)) and np.array_equal(got, dev.gcode_order(ends))
    with pytest.raises(OripError):
        dev.gcode_order(None, n + 1)


def test_order_large_pair_by_pair(dev):
    """60 000 uniformly spread paths: the reference needs minutes for 20 000 and is quadratic.  The result is a permutation, and for EVERY step k and EVERY
    path i chosen later than k, (L1(cursor_k, first_i), i) > (d_k, chosen_k): 1.8e9 pair tests in blocked numpy (14 s on one CPU core), nothing sampled."""
    rng = np.random.default_rng(60000)
    n = 60000
    e = np.concatenate([rng.integers(0, 8400, (n, 1)), rng.integers(0, 11880, (n, 1)), rng.integers(0, 8400, (n, 1)), rng.integers(0, 11880, (n, 1))], 1)
    got = dev.gcode_order(e)
    assert np.array_equal(np.sort(got), np.arange(n))
    assert D.order_violations(e, got) == 0
    assert D.order_violations(e, np.concatenate([got[:30000], got[30001:30002], got[30000:30001], got[30002:]])) > 0       # the check sees a swap


# ------------------------------------------------------------------ pack
@pytest.mark.parametrize("tag", ["a", "b"])
def test_pack_equals_numpy_assembler_on_stage13_plots(dev, tag):
    """same pieces, three packers: orip_stream_pack on the resident codes against the doubles' two on the fetched ones, and all three the reference's file"""
    from orip import stream as ST
    from orip.config import canvas_size_px
    cfgd, layers = _layers_from_e2e(tag)
    cfg = _pipeline_config(cfgd)
    W, H = canvas_size_px(cfg)
    sc = ST.stream_config_from_pipeline(cfg)
    P, _ = ST.plan_layers(layers, W, H, sc, ST.load_color_maps(cfg))
    fetched = {}

    def codes_fn(moves):                                                    # fetched for the doubles; the device packs from its own resident copy
        off, fetched["codes"] = dev.stream_codes(moves)
        return off, None
    data, table, _ = ST.compile_plan(P, sc, dev, codes_fn=codes_fn)
    want = bytes(GS[f"e2e_{tag}_bin"])
    assert fill_bytes(table, fetched["codes"]) == want
    assert data == want
    assert D.pack_numpy(table, fetched["codes"]) == want


def test_pack_edges(dev):
    from orip import stream as ST
    from orip.device import OripError
    off, codes = dev.stream_codes(np.array([[0, 0, 5, 2], [5, 2, 5, 2], [5, 2, 0, 9]], np.int32))
    assert len(codes) == 12
    # pieces of one and two steps, a piece that only sets the speed, a speed byte above 0x7f is refused, service bytes between pieces
    T = ST.PieceTable(np.array([0, 1, 3, 5], np.int64), np.array([1, 2, 0, 7], np.int32), np.array([1, 3, 6, 8], np.int64), np.array([0x5c, -1, 0x4a, 0x7f], np.int32),
                      np.array([0, 5, 7, 13], np.int64), np.array([1, 2, 1, 0x3f], np.uint8), 1024)
    assert dev.stream_pack(T) == D.pack_numpy(T, codes) == fill_bytes(T, codes)
    E = ST.PieceTable(np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int32), np.array([0], np.int64), np.array([0x3f], np.uint8), 1024)
    assert dev.stream_pack(E) == bytes([0x3f]) + bytes(1023)
    for bad in (dict(code0=np.array([0, 1, 3, 6], np.int64)),            # reads past the resident codes
                dict(pos=np.array([1, 2, 6, 8], np.int64)),              # overlaps the piece before it
                dict(pos=np.array([1, 3, 6, 1021], np.int64)),           # leaves the stream
                dict(svc_pos=np.array([0, 5, 7, 1024], np.int64)),
                dict(cnt=np.array([1, -2, 0, 7], np.int32))):
        with pytest.raises(OripError):
            dev.stream_pack(ST.PieceTable(**{**T.__dict__, **bad}))


# ------------------------------------------------------------------ the whole tool
@pytest.mark.parametrize("i", range(len(MAIN_CASES)))
def test_tool_reproduces_reference_file(dev, i, tmp_path):
    """main([...]) with every step on the device: input file in, output file out, the reference's bytes"""
    from orip import gcode as GC
    name, args = MAIN_CASES[i]
    src = tmp_path / "in.gcode"; src.write_bytes(bytes(G[f"text_{name}"]))
    dst = tmp_path / "out.bin"
    GC.main([str(src), "-o", str(dst)] + list(args), device=dev)
    assert dst.read_bytes() == bytes(G[f"main_{i}_bin"]), (name, args)


@pytest.mark.parametrize("i", [0, 3, 18])
def test_script_on_disk(i, tmp_path):
    name, args = MAIN_CASES[i]
    src = tmp_path / "in.gcode"; src.write_bytes(bytes(G[f"text_{name}"]))
    r = subprocess.run([sys.executable, SCRIPT, str(src), "-o", str(tmp_path / "out.bin")] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "out.bin").read_bytes() == bytes(G[f"main_{i}_bin"])


def test_script_fails_loudly(tmp_path):
    """what the reference refuses: a non-finite coordinate under the pen, Ginf, a colour outside 0..7 -- non-zero exit, no stream"""
    for text, args in (("M3\nG1 X1e308 Y1\nG1 X2 Y2\n", ["--scale-x", "1e10"]), ("Ginf\nM3\nG1 X1 Y1\n", []), ("M3\nG1 X5 Y5\n", ["--color-index", "9"])):
        src = tmp_path / "in.gcode"; src.write_text(text)
        r = subprocess.run([sys.executable, SCRIPT, str(src), "-o", str(tmp_path / "out.bin")] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and not (tmp_path / "out.bin").exists(), (text, r.stdout, r.stderr)


def test_round_trip_through_stream_preview(dev):
    """decode what was produced with the stage-14 kernel: steps, pen-down segments, final position and the end byte agree with the plan's totals"""
    from orip import gcode as GC, stream_preview as SP
    opts = options_for(MAIN_CASES[0][1])
    data, info = GC.build_stream_from_gcode(bytes(G["text_drawing"]), opts, dev)
    assert data == bytes(G["main_0_bin"])
    W, H = info["target"]
    _, st = SP.preview(dev, data, W, H, invert_y=False)
    off, pts = dev.gcode_to_steps(*GC.parse_gcode(bytes(G["text_drawing"]))[:2], dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=10.0, W=W, H=H, invert_y=0))
    last = dev.gcode_order(np.concatenate([pts[off[:-1]], pts[off[1:] - 1]], 1))[-1]
    assert st["steps_total"] == info["steps"] and st["pen_down_segments"] == info["paths"] == len(off) - 1 and st["taps"] == 0
    assert (st["final_x"], st["final_y"]) == tuple(pts[off[last + 1] - 1]) and st["eof_seen"] == 1 and st["color_changes"] == 1
    assert st["off_canvas_draws"] == 0 and st["unknown_service_bytes"] == 0 and st["total_bytes"] == len(data) == info["bytes"]
