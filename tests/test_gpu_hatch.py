"""The hatch fill on the GPU: orip_svg_hatch (csrc/hatch.hip) against every call the reference's hatch_fill made (tests/golden/golden_hatch.npz), against the
numpy double (tests/hatch_double.py) on larger seeded drawings that reach each sort path and the long-edge chunks, every error return followed by a
successful call, the resident hand-off into orip_gcode_to_steps, the two scripts on disk with and without the options, and one drawing through the stream
preview.  Everything is equality: no comparison here has a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hatch_double as HD
from test_hatch_host import H, CASES, case, flags_of, svg_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
STEP_MAP = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=1.0, W=1 << 20, H=1 << 20, invert_y=0)


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def put(dev, groups, fit=True):
    """integer polygons, a list of groups of [n, 2] arrays, resident as line subpaths under the identity fit -> (off, points, group of every subpath)"""
    t = HD.polys_table(groups)
    n = sum(len(p) for g in groups for p in g)
    assert dev.svg_flatten(t, 1.0) == n
    if fit:
        dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    off, pts = dev.svg_paths()
    assert np.array_equal(pts, np.concatenate([p for g in groups for p in g]))
    return off, pts, t.fill_group


def hatch_lines(dev, n_sub):
    """the paths behind the first n_sub as integer rows (x0, y0, x1, y1)"""
    off, pts = dev.svg_paths()
    assert np.array_equal(np.diff(off[n_sub:]), np.full(len(off) - 1 - n_sub, 2))
    tail = pts[off[n_sub]:]
    assert np.array_equal(tail, np.rint(tail))
    return tail.astype(np.int64).reshape(-1, 4)


# ------------------------------------------------------------------ the reference's recorded calls
@pytest.mark.parametrize("name", CASES)
def test_hatch_matches_reference(dev, name):
    polys, spacing, inset, serp, want = case(name)
    off, pts, fg = put(dev, [polys])
    st = dev.svg_hatch(fg, 1.0, spacing, inset, flags_of(serp))
    assert st["segments"] == len(want) and st["groups"] == 1
    assert np.array_equal(hatch_lines(dev, len(polys)), want)
    o2, p2 = dev.svg_paths()
    assert np.array_equal(o2[:len(off)], off) and np.array_equal(p2[:len(pts)], pts)            # the outlines are still there, in front


# ------------------------------------------------------------------ larger drawings against the double
def many_groups(n_groups, seed, r_max=400):
    rng = np.random.default_rng(seed)
    return [[HD.star(rng, rng.integers(0, 8400), rng.integers(0, 11880), rng.integers(20, r_max), int(rng.integers(3, 24))) for _ in range(int(rng.integers(1, 4)))] for _ in range(n_groups)]


def against_double(dev, groups, spacing, inset, flags, spm=1.0, fill=None):
    off, pts, fg = put(dev, groups)
    if fill is not None:
        fg = np.asarray(fill, np.int32)
    want, wst = HD.hatch_segments(off, HD.quantise(pts, spm), fg, spacing, inset, flags)
    st = dev.svg_hatch(fg, spm, spacing, inset, flags)
    assert st == wst
    o2, p2 = dev.svg_paths()
    assert len(o2) == len(off) + len(want) and np.array_equal(p2[:len(pts)], pts)
    from svg_double import round4_python
    assert np.array_equal(p2[len(pts):], round4_python(want.reshape(-1, 2).astype(np.float64) / spm))
    return want, st


def test_many_small_groups_all_directions(dev):
    """20000 groups of 1-3 stars: rows of 2-64 crossings, the wave sort; empty groups and unfilled subpaths in between"""
    groups = many_groups(20000, 11)
    n_sub = sum(len(g) for g in groups)
    rng = np.random.default_rng(3)
    fg = np.repeat(np.arange(len(groups)), [len(g) for g in groups]).astype(np.int32)
    fg[rng.random(n_sub) < 0.1] = -1
    for flags in (HD.HORIZONTAL | HD.SERPENTINE, HD.VERTICAL, HD.HORIZONTAL | HD.VERTICAL | HD.SERPENTINE):
        want, st = against_double(dev, groups, 20, 3, flags, fill=fg)
        assert st["segments"] > 10 ** 5


def test_rows_for_every_sort_path_and_long_edges(dev):
    """one group of 2000 tall thin stars side by side: every row holds up to a few thousand crossings (block sort and segmented sort), every edge spans hundreds
    to thousands of rows (many chunks per edge); beside it groups whose rows stay in a wave"""
    rng = np.random.default_rng(5)
    tall = []
    for i in range(2200):
        s = HD.star(rng, 0, 0, 1000, int(rng.integers(3, 9)))
        tall.append(np.stack([s[:, 0] // 100 + 12 * i, s[:, 1] * 5 + 5000 + int(rng.integers(-3000, 3000))], 1))
    groups = [tall[:2000], tall[2000:2100], tall[2100:2106]] + many_groups(50, 9)
    for spacing, flags in ((3, HD.HORIZONTAL | HD.SERPENTINE), (40, HD.HORIZONTAL | HD.VERTICAL | HD.SERPENTINE)):
        against_double(dev, groups, spacing, 1, flags)
    # what the rows of the first three groups hold, from the double's own crossing counts: beyond 2048, 65..2048, and at most 64
    for g, (lo, hi) in zip(range(3), ((2049, 10 ** 9), (65, 2048), (2, 64))):
        polys = groups[g]
        o = np.concatenate([[0], np.cumsum([len(p) for p in polys])])
        seg, st = HD.hatch_segments(o, np.concatenate(polys), np.zeros(len(polys), np.int64), 3, 0, HD.HORIZONTAL)
        per_row = 2 * np.bincount(seg[:, 1] - seg[:, 1].min())
        assert lo <= per_row.max() and (g == 0 or per_row.max() <= hi), (g, per_row.max())
    assert max(np.ptp(p[:, 1]) for p in tall) > 64 * 3 * 10                                     # edges of more than ten chunks at spacing 3


def test_quantisation_and_steps_per_mm(dev):
    """coordinates that are not whole steps, ties among them, at 40 and 7.3 steps per mm: q = rint(v * spm), and the lines come back as round4(k / spm)"""
    rng = np.random.default_rng(17)
    groups = many_groups(300, 21)
    for spm in (40.0, 7.3, 5000.0):
        t = HD.polys_table([[p / spm + rng.choice([0.0, 0.5 / spm, 0.0125, 1e-4], p.shape) for p in g] for g in groups])
        dev.svg_flatten(t, 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
        off, pts = dev.svg_paths()
        want, wst = HD.hatch_segments(off, HD.quantise(pts, spm), t.fill_group, 20, 3, HD.HORIZONTAL | HD.SERPENTINE)
        assert dev.svg_hatch(t.fill_group, spm, 20, 3, HD.HORIZONTAL | HD.SERPENTINE) == wst and wst["segments"] > 1000
        o2, p2 = dev.svg_paths()
        from svg_double import round4_python
        mm = round4_python(want.reshape(-1, 2).astype(np.float64) / spm)
        assert np.array_equal(p2[len(pts):], mm) and np.array_equal(np.rint(mm * spm).astype(np.int64), want.reshape(-1, 2))     # four decimals name every step


# ------------------------------------------------------------------ error returns
def test_error_returns_leave_nothing_behind(dev):
    from orip.device import OripError
    polys, spacing, inset, serp, want = case("hole")
    F = flags_of(serp)
    dev.svg_flatten(HD.polys_table([polys]), 1.0)
    with pytest.raises(OripError):                                                              # flattened, not fitted
        dev.svg_hatch([0, 0], 1.0, spacing, inset, F)
    off, pts, fg = put(dev, [polys])
    before = dev.svg_paths()

    def refused(*a):
        with pytest.raises(OripError):
            dev.svg_hatch(*a)
        after = dev.svg_paths()
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    refused([0, 0, 0], 1.0, spacing, inset, F)                                                  # not the resident count
    refused([0], 1.0, spacing, inset, F)
    refused([0, 2], 1.0, spacing, inset, F); refused([-2, 0], 1.0, spacing, inset, F)            # group out of range
    refused(fg, 1.0, 0, inset, F); refused(fg, 1.0, spacing, -1, F)
    refused(fg, 1.0, spacing, inset, HD.SERPENTINE); refused(fg, 1.0, spacing, inset, 8 | F)
    for spm in (0.0, -1.0, 5000.5, np.inf, np.nan):
        refused(fg, spm, spacing, inset, F)
    st = dev.svg_hatch(fg, 1.0, spacing, inset, F)                                              # and then it works
    assert st["segments"] == len(want) and np.array_equal(hatch_lines(dev, 2), want)
    with pytest.raises(OripError):                                                              # a second time without a new flatten
        dev.svg_hatch(fg, 1.0, spacing, inset, F)
    assert np.array_equal(hatch_lines(dev, 2), want)

    def big(polys, spm, spacing, flags=HD.HORIZONTAL):
        off, pts, fg = put(dev, [polys])
        with pytest.raises(OripError):
            dev.svg_hatch(fg, spm, spacing, 0, flags)
        after = dev.svg_paths()
        assert np.array_equal(after[0], off) and np.array_equal(after[1], pts)
    tri = lambda h, k=0: np.array([[k, 0], [1000 - k, 0], [500, h]], np.int64)
    big([tri(300000)], 5000.0, 1)                                                               # 1.5e9 hatch units
    big([tri(7 * 10 ** 7)], 1.0, 1)                                                             # more than 2^26 lines
    big([tri(6 * 10 ** 7, k) for k in range(12)], 1.0, 1)                                       # 1.44e9 crossings in 6e7 lines
    # vertical fails after horizontal has succeeded: still nothing appended
    off, pts, fg = put(dev, [[np.array([[0, 0], [7 * 10 ** 7, 0], [7 * 10 ** 7, 50], [0, 50]], np.int64)]])
    with pytest.raises(OripError):
        dev.svg_hatch(fg, 1.0, 1, 0, HD.HORIZONTAL | HD.VERTICAL)
    after = dev.svg_paths()
    assert np.array_equal(after[0], off) and np.array_equal(after[1], pts)
    st = dev.svg_hatch(fg, 1.0, 1, 0, HD.HORIZONTAL)                                            # the same paths, the direction that fits
    assert st["segments"] == 50 and st["lines"] == 51
    off, pts, fg = put(dev, [case("hole")[0]])                                                  # and the context goes on as if nothing had happened
    assert dev.svg_hatch(fg, 1.0, spacing, inset, F)["segments"] == len(want) and np.array_equal(hatch_lines(dev, 2), want)
    off, pts, _ = put(dev, [case("hole")[0]])
    assert dev.svg_hatch([-1, -1], 1.0, spacing, inset, F) == {"groups": 0, "lines": 0, "crossings": 0, "segments": 0}
    assert np.array_equal(dev.svg_paths()[1], pts)


# ------------------------------------------------------------------ the resident hand-off
def test_resident_hand_off(dev):
    from orip.device import OripError
    for name in ("hole", "islands_empty_lines", "nested_overlapping"):
        polys, spacing, inset, serp, want = case(name)
        off, pts, fg = put(dev, [polys])
        st = dev.svg_hatch(fg, 1.0, spacing, inset, flags_of(serp))
        o2, p2 = dev.svg_paths()
        assert len(o2) - 1 == len(polys) + len(want) and int(o2[-1]) == len(pts) + 2 * len(want)
        with pytest.raises(OripError):
            dev.gcode_to_steps(None, None, STEP_MAP, n=len(polys))                                   # the count is the hatched one now
        soff, spts = dev.gcode_to_steps(None, None, STEP_MAP, n=len(o2) - 1)
        n = len(soff) - 1 - len(want)
        assert np.array_equal(spts[soff[n]:].reshape(-1, 4), want)                              # the reference's integers
        b = dev.gcode_to_steps(o2, p2, STEP_MAP)
        assert np.array_equal(b[0], soff) and np.array_equal(b[1], spts)
        m = dict(STEP_MAP, invert_y=1, H=2000)
        soff, spts = dev.gcode_to_steps(None, None, m, n=len(o2) - 1)
        mirrored = want.copy(); mirrored[:, [1, 3]] = 1999 - mirrored[:, [1, 3]]
        assert np.array_equal(spts[soff[len(soff) - 1 - len(want)]:].reshape(-1, 4), mirrored)


# ------------------------------------------------------------------ the whole tool
def test_tool_in_process_matches_the_doubles(dev):
    from orip import svg as SV
    import svg_double as SD
    from test_svg_host import options_for, svg_text
    from test_hatch_host import FILLS
    for text, args in ((svg_of(case("hole")[0]), ["--scale", "0.025", "--margin-mm", "0", "--hatch-spacing-mm", "0.5", "--hatch-inset-mm", "0.075"]),
                       (svg_text("elements"), ["--hatch-spacing-mm", "0.7", "--hatch-fill", "all", "--hatch-direction", "cross"]),
                       (svg_text("transforms"), ["--hatch-spacing-mm", "1.5", "--hatch-fill", "all", "--no-serpentine", "--steps-per-mm", "10", "--invert-y", "1"]),
                       (FILLS, ["--hatch-spacing-mm", "0.3", "--hatch-inset-mm", "0.1", "--hatch-direction", "vertical"])):
        o = options_for(args)
        want, winfo = SV.build_stream_from_svg(text, o, want_paths=True, **dict(SD.svg_doubles(), hatch_fn=HD.hatch_numpy))
        got, info = SV.build_stream_from_svg(text, o, dev, want_paths=True)
        assert info["hatch"] == winfo["hatch"] and info["hatch"]["segments"] > 0
        assert np.array_equal(info["fitted_paths"][0], winfo["fitted_paths"][0]) and np.array_equal(info["fitted_paths"][1], winfo["fitted_paths"][1])
        assert got == want
        assert SV.build_stream_from_svg(text, o, dev)[0] == want                                # the points never fetched


def test_scripts_on_disk(tmp_path):
    from orip import svg as SV
    import svg_double as SD
    from test_svg_host import G, ARGS, RUNS, options_for
    i = 0
    name, key = RUNS[i]
    src = tmp_path / "drawing.svg"; src.write_bytes(bytes(G[f"svg_{name}"]))
    run = lambda script, extra: subprocess.run([sys.executable, os.path.join(SCRIPTS, script), str(src)] + extra, capture_output=True, text=True, timeout=300)
    r = run("svg2stream.py", ["--no-preview"] + ARGS[key])                                      # without the options: the recorded run, byte for byte
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "drawing_stream.bin").read_bytes() == bytes(G[f"run_{i}_bin"]) and (tmp_path / "drawing.gcode").read_bytes() == bytes(G[f"run_{i}_gcode"])
    assert "hatch" not in r.stdout
    r = run("svg2gcode.py", ["-o", str(tmp_path / "only.gcode")])
    assert r.returncode == 0 and (tmp_path / "only.gcode").read_bytes() == bytes(G[f"run_{i}_gcode"])
    hatch = ["--hatch-spacing-mm", "0.5", "--hatch-fill", "all", "--hatch-direction", "cross"]
    want, winfo = SV.build_stream_from_svg(bytes(G[f"svg_{name}"]), options_for(ARGS[key] + hatch), want_paths=True, **dict(SD.svg_doubles(), hatch_fn=HD.hatch_numpy))
    text = SV.gcode_text(*winfo["fitted_paths"])
    r = run("svg2stream.py", ["--preview-render-width", "640", "--preview-render-height", "480"] + ARGS[key] + hatch)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "drawing_stream.bin").read_bytes() == want and (tmp_path / "drawing.gcode").read_text() == text and winfo["hatch"]["segments"] > 100
    assert "hatch: %d fill groups" % winfo["hatch"]["groups"] in r.stdout and (tmp_path / "drawing_stream_preview.png").exists()
    r = run("svg2gcode.py", ["-o", str(tmp_path / "h.gcode")] + hatch)
    assert r.returncode == 0 and (tmp_path / "h.gcode").read_text() == text
    for bad in (["--hatch-spacing-mm", "0.001"], ["--hatch-spacing-mm", "1", "--steps-per-mm", "6000"]):
        r = run("svg2stream.py", ["-o", str(tmp_path / "bad.bin"), "--gcode-output", str(tmp_path / "bad.gcode"), "--no-preview"] + bad)
        assert r.returncode != 0 and not (tmp_path / "bad.bin").exists() and not (tmp_path / "bad.gcode").exists()


def test_preview_shows_the_filled_area(dev):
    """a square with a square hole, hatched every step in both directions with no inset: in the preview every pixel inside the ring is drawn, none in the hole"""
    from orip import svg as SV, stream_preview as SP
    from test_svg_host import options_for
    ring = [np.array([[0, 0], [800, 0], [800, 800], [0, 800]], np.int64), np.array([[300, 300], [300, 500], [500, 500], [500, 300]], np.int64)]
    args = ["--scale", "0.025", "--margin-mm", "0", "--page-width-mm", "20", "--page-height-mm", "20", "--hatch-spacing-mm", "0.025", "--hatch-inset-mm", "0", "--hatch-direction", "cross"]
    data, info = SV.build_stream_from_svg(svg_of(ring), options_for(args), dev)
    assert tuple(info["target"]) == (800, 800) and info["hatch"]["segments"] > 1500
    rgb, st = SP.preview(dev, data, 800, 800, 800, 800, invert_y=True)
    ink = (rgb != 255).any(2)
    assert st["off_canvas_draws"] == 0 and ink[20:280, 20:780].all() and ink[520:780, 20:780].all() and ink[20:780, 20:280].all() and ink[20:780, 520:780].all()
    assert not ink[320:480, 320:480].any()
    plain, _ = SV.build_stream_from_svg(svg_of(ring), options_for(args[:8]), dev)
    rgb0, _ = SP.preview(dev, plain, 800, 800, 800, 800, invert_y=True)
    assert not (rgb0 != 255).any(2)[20:280, 20:780].any()                                       # hollow without the options
