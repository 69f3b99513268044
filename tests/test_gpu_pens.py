"""The pens on the GPU: orip_gcode_order_pens against what the reference's order_paths_nearest returned (tests/golden/golden_pens.npz), bit for bit, and
against the brute-force double of tests/pens_double.py on the smallest shapes that can break the kernel -- each with and without stroke reversal -- and on
a random plot in four groups; its agreement with orip_gcode_order; its argument checks; the two small fetches that carry a pen through the hatch and the
conversion to steps; and the whole tool on a drawing in four pens, in process and as the script on disk, against the host path run through the doubles
and through the stage-14 decoder.  No comparison has a tolerance and no recorded case is left out."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pens_double as PD
import hatch_double as HD
from test_pens_host import GP, ORDER_CASES, stream_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
TOP = 1 << 30


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def same(dev, ends, group, n_groups, start=(0, 0)):
    """the device equals the double, without and with reversal"""
    ends = np.asarray(ends, np.int32).reshape(-1, 4); group = np.asarray(group, np.int32)
    for reverse in (False, True):
        o, r = dev.gcode_order_pens(ends, group, n_groups, reverse, start)
        wo, wr = PD.order_pens_numpy(ends, group, n_groups, reverse, start)
        assert o.dtype == np.int32 and r.dtype == bool and len(o) == len(r) == len(ends)
        assert np.array_equal(o, wo) and np.array_equal(r, wr), (reverse, np.nonzero((o != wo) | (r != wr))[0][:5])
        assert reverse or not r.any()


# ------------------------------------------------------------------ the recorded reference
@pytest.mark.parametrize("name", ORDER_CASES)
def test_order_matches_reference(dev, name):
    ends, start = GP[f"ord_{name}_ends"], GP[f"ord_{name}_start"]
    o, r = dev.gcode_order_pens(ends, np.zeros(len(ends), np.int32), 1, True, tuple(start.tolist()))
    assert np.array_equal(o, GP[f"ord_{name}_order"]) and np.array_equal(r, GP[f"ord_{name}_rev"])


# ------------------------------------------------------------------ the smallest shapes that can break the kernel
def test_order_tiny(dev):
    o, r = dev.gcode_order_pens(np.zeros((0, 4), np.int32), np.zeros(0, np.int32), 3, True)
    assert len(o) == 0 and len(r) == 0
    same(dev, [[5, 5, 9, 1]], [0], 1)
    same(dev, [[5, 5, 9, 1]], [2], 4, start=(9, 1))                       # the far end is nearer: reversed
    same(dev, [[7, 3, 2, 8], [7, 3, 2, 8]], [0, 0], 1)
    same(dev, [[4, 4, 4, 4]], [0], 1)                                     # one closed path alone: the forward end wins on the key
    same(dev, [[4, 4, 4, 4], [4, 4, 4, 4]], [0, 0], 1, start=(4, 4))


def test_order_closed_among_open(dev):
    rng = np.random.default_rng(5)
    e = rng.integers(0, 300, (400, 4))
    closed = rng.random(400) < 0.4
    e[closed, 2:] = e[closed, :2]
    same(dev, e, np.zeros(400), 1)
    same(dev, e, rng.integers(0, 3, 400), 3, start=(150, 150))


def test_order_one_crowded_cell(dev):
    """3000 paths with all four coordinates equal: one cell far beyond the size the whole wave scans, ties by id alone, and with reversal every winner's other
    end sits in the same cell, now and then as its last entry"""
    same(dev, np.full((3000, 4), 77), np.zeros(3000), 1)
    same(dev, np.full((3000, 4), 77), np.arange(3000) % 2, 2)


@pytest.mark.parametrize("k", [64, 65])
def test_order_cell_at_the_whole_wave_threshold(dev, k):
    """k paths per group on one point, two groups: without reversal a cell of 64 entries (four lanes each) or 65 (the whole wave), with it 128 / 130"""
    same(dev, np.full((2 * k, 4), 77), np.repeat([0, 1], k), 2)
    rng = np.random.default_rng(k)
    same(dev, np.concatenate([np.full((2 * k, 2), 77), rng.integers(0, 1 << 20, (2 * k, 2))], 1), np.arange(2 * k) % 2, 2)      # far ends apart: more cells than one


def test_order_both_ends_in_one_cell(dev):
    """short strokes on a wide sheet: a path's two ends share a cell (the grid's cells are far wider than a stroke)"""
    rng = np.random.default_rng(6)
    a = np.stack([rng.integers(0, 8000, 600), rng.integers(0, 8000, 600)], 1)
    e = np.concatenate([a, a + rng.integers(0, 3, (600, 2))], 1)
    same(dev, e, np.zeros(600), 1)
    e2 = np.concatenate([a[:40] // 400, a[:40] // 400 + rng.integers(0, 2, (40, 2))], 1)             # few paths, few cells, many shared points
    same(dev, e2, np.zeros(40), 1)


def test_order_row_and_column(dev):
    rng = np.random.default_rng(7)
    x = rng.integers(0, 5000, (500, 2))
    same(dev, np.stack([x[:, 0], np.full(500, 9), x[:, 1], np.full(500, 9)], 1), np.zeros(500), 1, start=(2500, 4000))      # one row, the cursor far above it
    y = rng.integers(0, TOP + 1, (500, 2)); y[0] = (0, TOP)
    same(dev, np.stack([np.full(500, TOP), y[:, 0], np.full(500, TOP), y[:, 1]], 1), np.zeros(500), 1)                        # one column at x = 2^30


def test_order_empty_groups(dev):
    rng = np.random.default_rng(8)
    e = rng.integers(0, 2000, (300, 4))
    same(dev, e, rng.integers(1, 4, 300), 4)                              # the first group is empty
    same(dev, e, rng.integers(0, 3, 300), 4)                              # the last one is
    same(dev, e, np.full(300, 7), 8)                                      # all paths in the last of 8
    same(dev, e, rng.choice([0, 63], 300), 64)                            # the most groups there can be, 62 of them empty


def test_order_groups_with_identical_points(dev):
    rng = np.random.default_rng(9)
    e = rng.integers(0, 1000, (250, 4))
    same(dev, np.concatenate([e, e]), np.repeat([0, 1], 250), 2)          # a candidate of the other group sits on every point
    same(dev, np.concatenate([e, e]), np.repeat([1, 0], 250), 2)


def test_order_group_far_away(dev):
    """the second group lies 2^29 steps from where the first one ends: the first search of the group starts outside its box"""
    rng = np.random.default_rng(10)
    a, b = rng.integers(0, 3000, (200, 4)), rng.integers(0, 3000, (200, 4)) + (1 << 29)
    same(dev, np.concatenate([a, b]), np.repeat([0, 1], 200), 2)
    same(dev, np.concatenate([a, b]), np.repeat([1, 0], 200), 2)
    b[:, 1] -= 1 << 29; b[:, 3] -= 1 << 29                                # far in x only
    same(dev, np.concatenate([a, b]), np.repeat([0, 1], 200), 2, start=(TOP, TOP))


# ------------------------------------------------------------------ the existing kernel
def test_order_agrees_with_gcode_order(dev):
    from test_gcode_host import G, conv_map, CONV_SETS
    ends = GP["ord_uniform_ends"]
    o, r = dev.gcode_order_pens(ends, np.zeros(len(ends), np.int32), 1)
    assert np.array_equal(o, dev.gcode_order(ends)) and not r.any()
    off, pts = dev.gcode_to_steps(G["conv_off"], G["conv_pts"], conv_map(CONV_SETS[0]))              # the resident polylines
    n = len(off) - 1
    assert n > 1
    o, r = dev.gcode_order_pens(None, np.zeros(n, np.int32), 1, n=n)
    assert np.array_equal(o, dev.gcode_order(None, n)) and not r.any()
    ends = np.concatenate([pts[off[:-1]], pts[off[1:] - 1]], 1)
    grp = np.arange(n) % 3
    for got, want in zip(dev.gcode_order_pens(None, grp, 3, True, n=n), PD.order_pens_numpy(ends, grp, 3, True)):
        assert np.array_equal(got, want)


# ------------------------------------------------------------------ random input
@pytest.fixture(scope="module")
def random_case():
    rng = np.random.default_rng(12)
    n = 12000
    ends = np.stack([rng.integers(0, 8400, n), rng.integers(0, 11880, n), rng.integers(0, 8400, n), rng.integers(0, 11880, n)], 1).astype(np.int32)
    grp = rng.integers(0, 4, n).astype(np.int32)
    return ends, grp, PD.order_pens_numpy(ends, grp, 4, True)


def test_order_random_four_groups(dev, random_case):
    ends, grp, (wo, wr) = random_case
    o, r = dev.gcode_order_pens(ends, grp, 4, True)
    assert np.array_equal(o, wo) and np.array_equal(r, wr)
    assert 0.3 < r.mean() < 0.7                                           # about every other stroke is nearer by its far end


# ------------------------------------------------------------------ bad arguments
def test_order_bad_arguments(dev):
    from orip.device import OripError
    e = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.int32)
    for ends, grp, ng, start in ((e, [0, 2], 2, (0, 0)), (e, [0, -1], 2, (0, 0)),                  # a group out of range
                                 (np.array([[1, 2, 3, TOP + 1], [5, 6, 7, 8]]), [0, 0], 1, (0, 0)), (np.array([[1, -2, 3, 4], [5, 6, 7, 8]]), [0, 0], 1, (0, 0)),
                                 (e, [0, 0], 0, (0, 0)), (e, [0, 0], 65, (0, 0)), (e, [0, 0], 1, (-1, 0)), (e, [0, 0], 1, (0, TOP + 1))):
        with pytest.raises(OripError):
            dev.gcode_order_pens(ends, grp, ng, True, start)
    off, _ = dev.gcode_to_steps(np.array([0, 2, 4]), np.array([[0.0, 0.0], [5.0, 1.0], [2.0, 2.0], [3.0, 3.0]]),
                                dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=10.0, W=400, H=300, invert_y=0))
    assert len(off) == 3
    with pytest.raises(OripError):                                        # three asked for, two resident
        dev.gcode_order_pens(None, [0, 0, 0], 1, n=3)
    assert dev.gcode_order_pens(None, [0, 0], 1, n=2)[0].tolist() == [0, 1]     # and the context is still good


# ------------------------------------------------------------------ the two fetches
def test_steps_source(dev):
    from test_gcode_host import conv_map, CONV_SETS
    m = conv_map(CONV_SETS[0])
    off, pts = dev.gcode_to_steps(np.array([0, 0, 1, 1, 3, 3]), np.array([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]]), m)      # the input of test_to_steps_edges
    assert np.array_equal(off, [0, 2]) and dev.gcode_steps_source(1).tolist() == [3]
    rng = np.random.default_rng(13)
    lens = rng.integers(0, 5, 300)
    o = np.concatenate([[0], np.cumsum(lens)])
    p = np.repeat(rng.uniform(0, 200, (300, 2)), lens, axis=0) + rng.normal(0, 0.04, (int(o[-1]), 2))
    S = PD.StepsWithSource()
    w_off, _ = S.steps(o, p, m)
    g_off, _ = dev.gcode_to_steps(o, p, m)
    assert np.array_equal(g_off, w_off) and 0 < len(S.src) < 300 and np.array_equal(dev.gcode_steps_source(len(g_off) - 1), S.src)


def test_hatch_groups(dev):
    """two fill groups under caller's numbers that are not their ranks, both directions: the device names the group of every line as the double counts them"""
    polys = [[np.array([[0, 0], [400, 0], [400, 300], [0, 300]])], [np.array([[500, 100], [900, 100], [700, 500]]), np.array([[100, 600], [300, 600], [200, 900]])]]
    t = HD.polys_table(polys)
    fg = np.where(t.fill_group == 0, 2, 1).astype(np.int32)              # the first polygon is group 2, the other two group 1
    prm = {"spacing": 16, "inset": 5, "flags": HD.HORIZONTAL | HD.VERTICAL | HD.SERPENTINE, "steps_per_mm": 1.0}
    dev.svg_flatten(t, 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    st = dev.svg_hatch(fg, prm["steps_per_mm"], prm["spacing"], prm["inset"], prm["flags"])
    H = PD.HatchWithGroups()
    off, pts = dev.svg_paths(t.n_sub + st["segments"])
    _, wst = H.hatch((off[:t.n_sub + 1], pts[:off[t.n_sub]]), fg, prm)
    assert st == wst and st["segments"] > 50
    got = dev.svg_hatch_groups(st["segments"])
    assert np.array_equal(got, H.groups) and set(got.tolist()) == {1, 2}


# ------------------------------------------------------------------ the whole tool
def decode(dev, data, info):
    from orip import stream_preview as SP
    W, H = info["target"]
    return SP.preview(dev, data, W, H, 320, 240, invert_y=True)[1]


def test_tool_in_process(dev):
    from orip import svg as SV
    o = stream_options(PD.TOOL_PEN_ARGS)
    want, winfo = SV.build_stream_from_svg(PD.TOOL_SVG, o, want_paths=True, **PD.pens_doubles())
    got, info = SV.build_stream_from_svg(PD.TOOL_SVG, o, dev, want_paths=True)
    assert got == want and info["pens"] == winfo["pens"] and np.array_equal(info["path_pens"], winfo["path_pens"])
    assert all(k > 0 for k in info["pens"]["paths"][:4]) and info["pens"]["unmatched"] == 1 and info["pens"]["reversed"] > 0
    st = decode(dev, got, info)
    assert st["color_changes"] == sum(1 for k in info["pens"]["paths"] if k) == 4
    assert st["pen_down_segments"] == info["paths"] and st["steps_total"] == info["steps"] and st["eof_seen"] == 1 and st["off_canvas_draws"] == 0


def test_tool_unchanged_without_the_options(dev):
    from orip import svg as SV
    got, info = SV.build_stream_from_svg(PD.TOOL_SVG, stream_options(PD.TOOL_PLAIN_ARGS), dev)
    assert got == bytes(GP["tool_plain_stream"]) and "pens" not in info


def test_tool_scripts_on_disk(dev, tmp_path):
    from orip import svg as SV
    src = tmp_path / "drawing.svg"
    src.write_bytes(PD.TOOL_SVG)
    run = lambda script, args: subprocess.run([sys.executable, os.path.join(SCRIPTS, script)] + args, capture_output=True, text=True, timeout=300)
    want, winfo = SV.build_stream_from_svg(PD.TOOL_SVG, stream_options(PD.TOOL_PEN_ARGS), want_paths=True, **PD.pens_doubles())
    text = SV.gcode_text(*winfo["fitted_paths"], pens=winfo["path_pens"])
    r = run("svg2stream.py", [str(src), "--preview-render-width", "320", "--preview-render-height", "240"] + PD.TOOL_PEN_ARGS)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "drawing_stream.bin").read_bytes() == want and (tmp_path / "drawing.gcode").read_text() == text
    assert "[svg] pens: 0: " in r.stdout and (tmp_path / "drawing_stream_preview.png").exists()
    st = decode(dev, want, winfo)
    assert st["color_changes"] == 4 and st["pen_down_segments"] == winfo["paths"] and st["steps_total"] == winfo["steps"] and st["eof_seen"] == 1 and st["off_canvas_draws"] == 0
    # the G-code it wrote, through gcode2stream --tool-pens: the same pens, hence the same stream
    r = run("gcode2stream.py", [str(tmp_path / "drawing.gcode"), "-o", str(tmp_path / "again.bin"), "--tool-pens", "--allow-reverse"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "again.bin").read_bytes() == want and "[gcode] pens: 0: " in r.stdout
