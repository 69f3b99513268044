"""svg2stream on the GPU: every kernel of csrc/svg.hip against the numpy double (tests/svg_double.py) and against the reference's recorded fit values, the
error returns, the resident hand-off into orip_gcode_to_steps, the whole tool in process and as the scripts on disk against the recorded reference streams
and G-code texts, and a round trip through the stream preview.  Device against double is equality: no comparison here has a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import svg_double as SD
from test_svg_host import G, ARGS, RUNS, NAMES, FIT_COUNT, svg_text, options_for, table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def same(a, b):
    """offsets equal, points equal as numbers (0.0 == -0.0), shapes equal"""
    return np.array_equal(a[0], b[0]) and a[1].shape == b[1].shape and np.array_equal(a[1], b[1])


def polyline_table(pts):
    """the points as ONE subpath of lines under a matrix that leaves them as they are: how arbitrary values get onto the device"""
    from orip.svg import SegmentTable
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    ctrl = np.stack([p[:-1], p[1:], p[1:], p[1:]], 1)
    return SegmentTable(np.ones(len(ctrl), np.int32), ctrl, np.zeros(len(ctrl), np.int32), np.array([0, len(ctrl)], np.int64), np.zeros(1, np.uint8),
                        np.array([[1.0, 0.0, 0.0, -1.0, 0.0, 0.0]]), 0.0)


def seeded_table(n_seg=200000, seed=7):
    """mixed lines, quadratics and cubics in chains of 1..6 under 40 random matrices; among them curves whose control points all coincide, collinear ones,
    and quadratics under the identity whose second difference sits exactly on, just below and just above n^2 k for the tolerance 0.25 (k = 1)"""
    from orip.svg import SegmentTable
    rng = np.random.default_rng(seed)
    kind = rng.integers(1, 4, n_seg).astype(np.int32)
    ctrl = rng.uniform(-50, 150, (n_seg, 4, 2))
    lens = rng.integers(1, 7, n_seg)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), n_seg)) + 1].tolist()
    lens[-1] -= sum(lens) - n_seg
    sub_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    mats = np.concatenate([[[1.0, 0.0, 0.0, -1.0, 0.0, 0.0]], rng.normal(0, 1.2, (40, 6))])
    mat = np.repeat(rng.integers(1, 41, len(lens)), lens).astype(np.int32)
    end = ctrl[np.arange(n_seg), np.where(kind <= 1, 1, kind)]
    inner = np.ones(n_seg, bool); inner[sub_off[:-1]] = False
    ctrl[inner, 0] = end[np.nonzero(inner)[0] - 1]                                      # chains; the device does not ask for it, and the families below break them again
    deg = rng.choice(n_seg, 3000, replace=False)
    ctrl[deg[:1000]] = ctrl[deg[:1000], :1]                                             # a point
    t = rng.uniform(-1, 2, (1000, 4, 1))
    ctrl[deg[1000:2000]] = ctrl[deg[1000:2000], :1] + t * (ctrl[deg[1000:2000], 3:] - ctrl[deg[1000:2000], :1])   # collinear, handles beyond the ends too
    b = deg[2000:]
    n = rng.integers(1, 200, 1000).astype(np.float64)
    d = n * n
    d[0::3] = np.nextafter(d[0::3], 0); d[1::3] = np.nextafter(d[1::3], np.inf)
    kind[b] = 2; mat[b] = 0
    ctrl[b] = 0.0; ctrl[b, 2, 0] = d; ctrl[b, 3, 0] = d
    return SegmentTable(kind, ctrl, mat, sub_off, np.zeros(len(lens), np.uint8), mats, 0.0), b, n


# ------------------------------------------------------------------ flatten, bbox
@pytest.mark.parametrize("name", NAMES)
def test_flatten_and_bbox_match_double_on_fixtures(dev, name):
    t = table_of(name)
    for tol in (0.5, 0.03, 1e-3):
        want = SD.flatten_numpy(t, tol)
        total = dev.svg_flatten(t, tol)
        got = dev.svg_paths()
        assert total == len(want[1]) and same(got, want), (name, tol)
        if t.n_seg:
            assert dev.svg_bbox() == SD.bbox_numpy(want)
            P = SD.transform(t)                                                            # the first and last point of a subpath: transformed control end points, exactly
            assert np.array_equal(got[1][got[0][:-1]], P[t.sub_off[:-1], 0]) and np.array_equal(got[1][got[0][1:] - 1], P[np.arange(t.n_seg), np.where(t.kind <= 1, 1, t.kind)][t.sub_off[1:] - 1])


def test_flatten_large_seeded_table(dev):
    t, b, n = seeded_table()
    tol = 0.25
    want = SD.flatten_numpy(t, tol)
    total = dev.svg_flatten(t, tol)
    got = dev.svg_paths()
    assert total == len(want[1]) > 10 ** 6 and same(got, want)
    assert dev.svg_bbox() == SD.bbox_numpy(want)
    cnt = SD.piece_counts(t.kind, SD.transform(t), tol)[b]                                 # the boundary family did what it was built for
    assert np.array_equal(cnt[2::3], n[2::3]) and np.array_equal(cnt[1::3], n[1::3] + 1) and np.array_equal(cnt[0::3], np.maximum(n[0::3], 1)) and (n[0::3] > 1).any()
    got2 = (dev.svg_flatten(t, 2.0), dev.svg_paths())[1]                                   # a second run into the same buffers, with fewer points
    assert same(got2, SD.flatten_numpy(t, 2.0))


# ------------------------------------------------------------------ fit
@pytest.mark.parametrize("i", range(FIT_COUNT))
def test_fit_matches_reference(dev, i):
    """every value the reference's scale_and_offset_gcode wrote, read back as float64"""
    pts = G["fit_in"]
    assert dev.svg_flatten(polyline_table(pts), 1.0) == len(pts)
    off, raw = dev.svg_paths()
    assert np.array_equal(raw, pts) and dev.svg_bbox() == tuple(G["fit_box"].tolist())
    dev.svg_fit(*G[f"fit_{i}_params"].tolist())
    _, got = dev.svg_paths()
    assert np.array_equal(got, G[f"fit_{i}_out"])


def test_fit_matches_double_on_seeded_values(dev):
    rng = np.random.default_rng(99)
    v = np.concatenate([rng.uniform(-500, 500, 600000), rng.uniform(-1e-3, 1e-3, 100000), rng.integers(-10 ** 7, 10 ** 7, 200000) / 1e4 + 5e-5,
                        rng.integers(-10 ** 6, 10 ** 6, 100000) / 32.0, np.arange(-9999, 10000, 2) / 32.0, np.arange(-5000, 5000) / 1e4 + 5e-5, [5e-05, -5e-05, 0.0, 1e-300, -1e-300]])
    if len(v) % 2:
        v = np.concatenate([v, [0.0]])
    pts = v.reshape(-1, 2)
    assert len(v) > 10 ** 6
    for prm in ((1.0, 1.0, 0.0, 0.0), (0.7311, -1.37, 12.3456789, -0.000049), (3.0, 1.0 / 3.0, 5e-05, 1e-4)):
        dev.svg_flatten(polyline_table(pts), 1.0)
        dev.svg_fit(*prm)
        _, got = dev.svg_paths()
        _, want = SD.fit_numpy((None, pts), *prm)
        assert np.array_equal(got, want) and got.tobytes() == want.tobytes(), prm              # the sign of a zero included


# ------------------------------------------------------------------ error returns
def test_error_returns(dev):
    """each through an input that the size and finiteness checks reject: the values that are not finite and the fit beyond 1e9 before any kernel sees
    them, the over-long curve by the counting kernel, which only raises a flag -- no point of it is ever emitted"""
    from orip.device import OripError
    from orip.svg import SegmentTable

    def T(ctrl, kind=2, mats=((1.0, 0, 0, -1.0, 0, 0),), mat=0, sub=(0, 1)):
        return SegmentTable(np.array([kind], np.int32), np.array(ctrl, np.float64).reshape(1, 4, 2), np.array([mat], np.int32), np.array(sub, np.int64), np.zeros(1, np.uint8),
                            np.array(mats, np.float64), 0.0)
    good = T([0, 0, 1, 1, 2, 0, 2, 0])
    bad = [(T([0, 0, 0, 0, 1e12, 0, 1e12, 0]), 1e-3),                                       # 1.6e7 pieces
           (T([0, 0, np.inf, 0, 1, 0, 1, 0]), 1.0), (T([0, 0, np.nan, 0, 1, 0, 1, 0], kind=3), 1.0),
           (T([0, 0, 1, 1, 2, 0, 2, 0], mats=((1.0, 0, 0, np.nan, 0, 0),)), 1.0),
           (T([0, 0, 1e300, 1, 2, 0, 2, 0], mats=((1e300, 0, 0, 1.0, 0, 0),)), 1.0),         # finite going in, not finite after the matrix
           (good, 0.0), (good, -1.0), (good, np.inf), (good, np.nan),
           (T([0, 0, 1, 1, 2, 0, 2, 0], kind=4), 1.0), (T([0, 0, 1, 1, 2, 0, 2, 0], mat=1), 1.0), (T([0, 0, 1, 1, 2, 0, 2, 0], sub=(0, 0, 1)), 1.0)]
    for t, tol in bad:
        with pytest.raises(OripError):
            dev.svg_flatten(t, tol)
        with pytest.raises(OripError):                                                      # and nothing is left behind
            dev.svg_bbox()
        with pytest.raises(OripError):
            dev.gcode_to_steps(None, None, dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=10.0, W=100, H=100, invert_y=0), n=1)
    assert dev.svg_flatten(T([0, 0, 0, 0, 65536.0 ** 2, 0, 65536.0 ** 2, 0]), 0.25) == 65537   # exactly 2^16 pieces pass
    with pytest.raises(OripError):
        dev.svg_flatten(T([0, 0, 0, 0, np.nextafter(65536.0 ** 2, np.inf), 0, 0, 0]), 0.25)
    dev.svg_flatten(good, 0.01)
    before = dev.svg_paths()
    for prm in ((1e9, 1.0, 0.0, 0.0), (1.0, 1.0, 0.0, -1e9), (np.inf, 1.0, 0.0, 0.0), (1.0, np.nan, 0.0, 0.0), (1e308, 1.0, 1e308, 0.0)):
        with pytest.raises(OripError):
            dev.svg_fit(*prm)
        assert same(dev.svg_paths(), before)                                                # refused before anything changed
    dev.svg_fit(4e8, 1.0, 0.0, 0.0)                                                         # 8e8: inside
    assert dev.svg_paths()[1][:, 0].max() == 8e8
    empty = SegmentTable(np.zeros(0, np.int32), np.zeros((0, 4, 2)), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.uint8), np.array([[1.0, 0, 0, 1.0, 0, 0]]), 0.0)
    assert dev.svg_flatten(empty, 1.0) == 0
    with pytest.raises(OripError):
        dev.svg_bbox()                                                                      # an empty drawing has no box
    dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    assert dev.svg_paths()[0].tolist() == [0]


# ------------------------------------------------------------------ the resident hand-off
def test_resident_hand_off(dev):
    import ctypes as C
    from orip.device import OripError
    from orip.lib import GcodeMap
    t = table_of("elements")
    m = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=40.0, W=8400, H=11880, invert_y=0)
    for mm in (m, dict(m, invert_y=1, steps_per_mm=7.3, W=1533, H=2168), dict(m, steps_per_mm=2.0, W=300, H=300)):                 # the last one clamps part of the drawing
        dev.svg_flatten(t, 0.02)
        dev.svg_fit(1.4, 1.4, 12.0, -3.0)
        off, pts = dev.svg_paths()
        a = dev.gcode_to_steps(None, None, mm, n=t.n_sub)
        order = dev.gcode_order(None, len(a[0]) - 1)
        b = dev.gcode_to_steps(off, pts, mm)
        assert len(a[0]) > 5 and same(a, b) and np.array_equal(order, dev.gcode_order(np.concatenate([b[1][b[0][:-1]], b[1][b[0][1:] - 1]], 1)))
        assert same(dev.svg_paths(), (off, pts))                                            # the fitted paths are still there
    with pytest.raises(OripError):
        dev.gcode_to_steps(None, None, m, n=t.n_sub + 1)
    with pytest.raises(OripError):                                                          # one pointer alone is neither form
        dev._ck(dev.L.orip_gcode_to_steps(dev.h, None, pts.ctypes.data_as(C.c_void_p), t.n_sub, C.byref(GcodeMap(**m)), C.byref(C.c_int64(0)), C.byref(C.c_int64(0))))


# ------------------------------------------------------------------ the whole tool
@pytest.mark.parametrize("i", range(len(RUNS)))
def test_tool_reproduces_reference_stream(dev, i):
    from orip import svg as SV
    name, key = RUNS[i]
    data, info = SV.build_stream_from_svg(svg_text(name), options_for(ARGS[key]), dev, want_paths=True)
    assert data == bytes(G[f"run_{i}_bin"]), (name, key)
    off, pts = info["fitted_paths"]
    assert np.array_equal(off, G[f"run_{i}_off"]) and np.array_equal(pts, G[f"run_{i}_pts"])
    assert SV.gcode_text(off, pts).encode() == bytes(G[f"run_{i}_gcode"])
    if "scale" in info:
        assert list(info["scale"]) + list(info["bbox"]) + [info["tol_raw"], info["flattens"]] == G[f"run_{i}_fit"].tolist()
    data2, _ = SV.build_stream_from_svg(svg_text(name), options_for(ARGS[key]), dev)          # the points never fetched
    assert data2 == data


@pytest.mark.parametrize("i", [0, 3, 9, 24, 28])
def test_scripts_on_disk(i, tmp_path):
    """svg2stream.py and svg2gcode.py as child processes: the recorded stream and G-code text, the preview at the requested size, and the same stream again
    from gcode2stream.py on the G-code file just written"""
    from PIL import Image
    from orip import svg as SV
    name, key = RUNS[i]
    o = options_for(ARGS[key])
    src = tmp_path / "drawing.svg"; src.write_bytes(bytes(G[f"svg_{name}"]))
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "svg2stream.py"), str(src), "--preview-render-width", "640", "--preview-render-height", "480"] + ARGS[key],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    stream = (tmp_path / "drawing_stream.bin").read_bytes()
    assert stream == bytes(G[f"run_{i}_bin"]) and (tmp_path / "drawing.gcode").read_bytes() == bytes(G[f"run_{i}_gcode"])
    assert Image.open(tmp_path / "drawing_stream_preview.png").size == (640, 480)
    go = SV.gcode_options(o)
    fwd = ["--steps-per-mm", str(o.steps_per_mm), "--invert-y", str(o.invert_y), "--color-index", str(o.color_index), "--speed-scale", str(o.speed_scale),
           "--target-width-steps", str(go.target_width_steps), "--target-height-steps", str(go.target_height_steps)] + (["--no-reorder"] if o.no_reorder else [])
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "gcode2stream.py"), str(tmp_path / "drawing.gcode"), "-o", str(tmp_path / "again.bin")] + fwd,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and (tmp_path / "again.bin").read_bytes() == stream
    fit = [a for k in ("--page-width-mm", "--page-height-mm", "--margin-mm", "--scale", "--scale-x", "--scale-y", "--tolerance-mm", "--steps-per-mm") if k in ARGS[key]
           for a in ARGS[key][ARGS[key].index(k):ARGS[key].index(k) + 2]]
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "svg2gcode.py"), str(src), "-o", str(tmp_path / "only.gcode"), "--passes", "1", "--cutting-speed", "900"] + fit,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "only.gcode").read_bytes() == bytes(G[f"run_{i}_gcode"])


def test_script_options_and_failures(tmp_path):
    src = tmp_path / "d.svg"; src.write_bytes(bytes(G["svg_commands_abs"]))
    i = RUNS.index(["commands_abs", "coarse"])
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "svg2stream.py"), str(src), "-o", str(tmp_path / "s.bin"), "--gcode-output", str(tmp_path / "g.nc"), "--no-preview"] + ARGS["coarse"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and (tmp_path / "s.bin").read_bytes() == bytes(G[f"run_{i}_bin"]) and (tmp_path / "g.nc").read_bytes() == bytes(G[f"run_{i}_gcode"])
    assert not (tmp_path / "d_stream_preview.png").exists()
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "svg2gcode.py"), str(src), "-o", str(tmp_path / "p.gcode"), "--steps-per-mm", "10", "--passes", "3"], capture_output=True, text=True, timeout=300)
    one = bytes(G[f"run_{i}_gcode"]).decode()
    assert r.returncode == 0 and (tmp_path / "p.gcode").read_text() == one + 2 * one[len("G21\nG90\nM5\n"):]
    for args in (["--speed-scale", "0"], ["--tolerance-mm", "-1"], ["--color-index", "9"], ["--scale", "1e12"]):
        r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "svg2stream.py"), str(src), "-o", str(tmp_path / "bad.bin"), "--gcode-output", str(tmp_path / "bad.gcode"), "--no-preview"] + args,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and not (tmp_path / "bad.bin").exists() and not (tmp_path / "bad.gcode").exists(), (args, r.stdout, r.stderr)


def test_round_trip_through_stream_preview(dev):
    from orip import svg as SV, stream_preview as SP
    i = 0
    name, key = RUNS[i]
    data, info = SV.build_stream_from_svg(svg_text(name), options_for(ARGS[key]), dev)
    assert data == bytes(G[f"run_{i}_bin"])
    W, H = info["target"]
    rgb, st = SP.preview(dev, data, W, H, 800, 600, invert_y=True)
    assert rgb.shape == (600, 800, 3) and (rgb != 255).any()
    assert st["pen_down_segments"] == info["paths"] == 10 and st["steps_total"] == info["steps"] and st["eof_seen"] == 1 and st["taps"] == 0
    assert st["off_canvas_draws"] == 0 and st["unknown_service_bytes"] == 0 and st["total_bytes"] == len(data)
