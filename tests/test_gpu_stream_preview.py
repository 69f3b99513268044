"""Stage 14 (stream preview) on the GPU: the HIP kernels behind orip_stream_preview against the reference previewer's statistics and draw calls
(tests/golden/golden_stream_preview.npz) and bit for bit against the numpy double (tests/stream_preview_double.py); edge cases, a 16 MB stream
with heavy overdraw, argument checks, and the drop-in stage scripts 13 -> 14 on disk."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from util import load
import stream_preview_double as D
from test_stream_preview_host import G, RUNS, args_of, golden_rgb_from_calls
from test_stream_host import _layers_from_e2e

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omnirevolve-image-processor_amd")
GS = load("golden_stream.npz")


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def run_dev(dev, data, W, H, rw, rh, inv=True, clip=True, taps=True, bg=True, pal=((255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0))):
    from orip import stream_preview as SP
    return dev.stream_preview(np.frombuffer(bytes(data), np.uint8), W, H, rw, rh, SP.flags_of(inv, clip, taps, bg), pal, SP.tap_radius())


@pytest.mark.parametrize("run", RUNS)
def test_statistics_and_image(dev, run):
    data, W, H, rw, rh, inv, clip, taps, bg, pal = args_of(run)
    rgb, st = run_dev(dev, data, W, H, rw, rh, inv, clip, taps, bg, pal)
    assert [st[k] for k in D.FIELDS] == G[f"{run}_stats"].tolist()
    want, st2 = D.preview(data, W, H, rw, rh, inv, clip, taps, bg, pal)
    assert st == st2
    assert rgb.shape == (rh, rw, 3) and np.array_equal(rgb, want)
    if float(G[f"{run}_scale"]) <= 1.0:                      # non-disc pixels: what the previewer's line calls set
        ref, mask = golden_rgb_from_calls(run, rw, rh, bg)
        assert np.array_equal(rgb[mask], ref[mask])


@pytest.mark.parametrize("data", [b"", b"\x3f", b"\x3f\x02\x81\x81", b"\x81", b"\x02", b"\x03", b"\x00", b"\xc9\x02\xc9\x3f"], ids=repr)
def test_edge_cases(dev, data):
    for W, H, rw, rh, inv, clip in ((600, 450, 400, 300, True, True), (3, 3, 400, 300, False, False)):
        rgb, st = run_dev(dev, data, W, H, rw, rh, inv, clip)
        want, st2 = D.preview(data, W, H, rw, rh, inv, clip)
        assert st == st2 and np.array_equal(rgb, want)
    if data[:1] == b"\x3f":
        assert st["eof_seen"] == 1 and st["tail_after_eof"] == len(data) - 1 and st["commands"] == 0 and st["service_bytes"] == 1


def overdraw_stream(nbytes, seed):
    """pen down most of the time, short random walks: every pixel of a few hundred is drawn by many commands of many workgroups"""
    rng = np.random.default_rng(seed)
    b = (0x80 | rng.integers(0, 128, nbytes)).astype(np.uint8)
    u = rng.random(nbytes)
    b[u < 0.02] = 0x02
    b[(u >= 0.02) & (u < 0.025)] = 0x01
    m = (u >= 0.025) & (u < 0.035)
    b[m] = (0x08 + rng.integers(0, 8, int(m.sum()))).astype(np.uint8)
    b[(u >= 0.035) & (u < 0.0351)] = 0x03
    b[(u >= 0.0351) & (u < 0.036)] = 0x44
    b[(u >= 0.036) & (u < 0.0362)] = 0x30
    b[:10000] = 0xC9                                        # pen up to (20000, 20000) first: double NE steps
    b[nbytes - 1000] = 0x3F                                 # EOF with a tail
    return b.tobytes()


def test_large_stream_overdraw_exact_and_repeatable(dev):
    data = overdraw_stream(16 << 20, 11)
    W, H, rw, rh = 40000, 40000, 1200, 900                   # step_scale 0.0225: 24 M steps within a few hundred pixels of the centre
    a, st = run_dev(dev, data, W, H, rw, rh)
    b, st_b = run_dev(dev, data, W, H, rw, rh)
    assert st == st_b and a.tobytes() == b.tobytes()
    want, st2 = D.preview(data, W, H, rw, rh)
    assert st == st2 and st["tail_after_eof"] == 999
    assert np.array_equal(a, want)
    assert (a != 255).any(-1).sum() > 1000 and st["off_canvas_draws"] == 0


def test_invalid_arguments(dev):
    import ctypes as C
    from orip.device import OripError
    d = np.zeros(16, np.uint8)
    ok = dict(data=d, W=600, H=450, rw=400, rh=300, flags=15, palette=np.zeros((4, 3), np.uint8), tap_radius=5)
    for bad in (dict(W=0), dict(H=-3), dict(rw=0), dict(rh=-1), dict(rw=16385), dict(rh=1 << 20), dict(tap_radius=0), dict(tap_radius=5000), dict(flags=16)):
        with pytest.raises(OripError):
            dev.stream_preview(**{**ok, **bad})
    with pytest.raises(OripError):                           # no preview to fetch after a failure
        dev._ck(dev.L.orip_stream_preview_fetch(dev.h, d.ctypes.data_as(C.c_void_p)))
    st = np.zeros(17, np.int64); pal = np.zeros(12, np.uint8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    assert dev.L.orip_stream_preview(dev.h, P(d), (1 << 31) - 1, 600, 450, 400, 300, 15, P(pal), 5, P(st)) != 0     # beyond int32 positions
    assert dev.L.orip_stream_preview(dev.h, None, 16, 600, 450, 400, 300, 15, P(pal), 5, P(st)) != 0
    assert dev.L.orip_stream_preview(dev.h, P(d), -1, 600, 450, 400, 300, 15, P(pal), 5, P(st)) != 0
    assert dev.L.orip_stream_preview(dev.h, P(d), 16, 600, 450, 400, 300, 15, None, 5, P(st)) != 0
    assert dev.L.orip_stream_preview(dev.h, P(d), 16, 600, 450, 400, 300, 15, P(pal), 5, None) != 0
    assert dev.L.orip_stream_preview_fetch(dev.h, None) != 0
    rgb, s = dev.stream_preview(**ok)                        # the context still works
    assert rgb.shape == (300, 400, 3) and s["total_bytes"] == 16


def _stage13_tree(out, tag="b"):
    cfgd, layers = _layers_from_e2e(tag)
    E = load(f"golden_e2e_{tag}.npz")
    full = dict(cfgd); full["output_dir"] = str(out)
    (out / "config.json").write_text(json.dumps(full))
    for name, _, ops in layers:
        (out / name).mkdir()
        with open(out / name / "ops.pkl", "wb") as f:
            pickle.dump(ops, f)
    (out / "vector_manifest.json").write_text(bytes(E["manifest_json"]).decode())


def _check_preview_files(out):
    from PIL import Image
    st = json.loads((out / "plot_stream_preview.json").read_text())
    assert st["taps"] == json.loads((out / "plot_stream.json").read_text())["taps"]
    data = (out / "plot_stream.bin").read_bytes()
    want, st2 = D.preview(data, 8400, 11880, 1200, 900)      # no stream_meta.json: 210 x 297 mm at 40 steps / mm
    assert st == st2 and [st[k] for k in D.FIELDS] == G["b_stage_stats"].tolist()
    assert np.array_equal(np.asarray(Image.open(out / "plot_stream_preview.png").convert("RGB")), want)


def test_stage_scripts_13_then_14_on_disk(tmp_path):
    out = tmp_path / "out"; out.mkdir()
    _stage13_tree(out)
    env = dict(os.environ, CONFIG_PATH=str(out / "config.json"))
    for script in ("13_build_stream.py", "14_preview_stream.py"):
        r = subprocess.run([sys.executable, os.path.join(PKG, "stages", script)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "=== Statistics ===" in r.stdout
    _check_preview_files(out)


def test_pipeline_runs_13_to_14(tmp_path):
    out = tmp_path / "out"; out.mkdir()
    _stage13_tree(out)
    r = subprocess.run([sys.executable, os.path.join(PKG, "stages", "pipeline.py"), "unused.png", "--output", str(out), "--start-step", "13", "--end-step", "14"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "[14/14] Preview stream" in r.stdout and "skipped" not in r.stdout
    _check_preview_files(out)


def test_command_line(tmp_path):
    from PIL import Image
    data = bytes(G["synth_none"])
    (tmp_path / "s.bin").write_bytes(data)
    r = subprocess.run([sys.executable, "-m", "orip.stream_preview", str(tmp_path / "s.bin"), "-o", str(tmp_path / "p.png"), "--canvas-w-steps", "600",
                        "--canvas-h-steps", "450", "--invert-y", "0", "--background-white", "0", "--render-width", "100", "--render-height", "700",
                        "--no-clip", "--c0", "#102030", "--c3", "y", "--stats-json", str(tmp_path / "s.json")], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    pal = ((16, 32, 48), (0, 255, 0), (0, 0, 255), (255, 255, 0))
    want, st = D.preview(data, 600, 450, 400, 700, invert_y=False, clip=False, background_white=False, palette=pal)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "p.png").convert("RGB")), want)
    assert json.loads((tmp_path / "s.json").read_text()) == st
    assert f"Total bytes: {len(data):,}".replace(",", " ") in r.stderr and f"Final position: ({st['final_x']}, {st['final_y']})" in r.stderr
