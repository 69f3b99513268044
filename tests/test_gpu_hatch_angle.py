"""The hatch at an angle on the GPU: orip_svg_hatch_angle (csrc/hatch_angle.hip) against the sequential double (tests/hatch_angle_double.py) on the smallest
drawings that reach each rule and each path of the kernels, every error return followed by a successful call, the resident hand-off, the tool in process and
on disk, and one drawing through the stream preview.  Everything is equality: the mm points, all five counts and the fetched groups."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hatch_double as HD
import hatch_angle_double as HA
from svg_double import round4_python

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "omnirevolve-image-processor_amd", "svg_to_stream")
STEP_MAP = dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=1.0, W=1 << 20, H=1 << 20, invert_y=0)
ANGLES = {0: (4096, 0), 90: (0, 4096), 45: (2896, 2896), 30: (3547, 2048), -60: (2048, -3547), 17.5: (3906, 1232)}
BOTH = HA.HORIZONTAL | HA.VERTICAL | HA.SERPENTINE
A = lambda *p: np.array(p, np.int64).reshape(-1, 2)


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def put(dev, groups):
    """integer polygons, a list of groups of [n, 2] arrays, resident as line subpaths under the identity fit -> (off, points, group of every subpath)"""
    t = HD.polys_table(groups)
    assert dev.svg_flatten(t, 1.0) == sum(len(p) for g in groups for p in g)
    dev.svg_fit(1.0, 1.0, 0.0, 0.0)
    off, pts = dev.svg_paths()
    assert np.array_equal(pts, np.concatenate([p for g in groups for p in g]))
    return off, pts, t.fill_group


def against_double(dev, groups, spacing, inset, u, flags, spm=1.0, fill=None):
    off, pts, fg = put(dev, groups)
    if fill is not None:
        fg = np.asarray(fill, np.int32)
    want, wst, wgrp, ks, _ = HA.hatch_lines_angle(off, HA.quantise(pts, spm), fg, spacing, inset, u, flags)
    st = dev.svg_hatch_angle(fg, spm, spacing, inset, u, flags)
    assert st == wst, (st, wst)
    o2, p2 = dev.svg_paths()
    assert len(o2) == len(off) + len(want) and np.array_equal(o2[:len(off)], off) and np.array_equal(np.diff(o2[len(off) - 1:]), np.full(len(want), 2))
    assert np.array_equal(p2[:len(pts)], pts)
    assert np.array_equal(p2[len(pts):], round4_python(want.reshape(-1, 2).astype(np.float64) / spm))
    assert np.array_equal(dev.svg_hatch_groups(st["segments"]), wgrp)
    return want, st, ks


# ------------------------------------------------------------------ the rule, shape by shape
def scene(dx=0, dy=0):
    """one group per situation of the rule.  At u = (4096, 0) and spacing 10 the lines are y = 10 k; at 45 degrees line 0 is y = x"""
    sq = lambda x, y, w: A([x, y], [x + w, y], [x + w, y + w], [x, y + w])
    g = [
        [A([3, 1], [97, 12], [31, 83])],                                                        # one triangle
        [A([200, 0], [260, 30], [320, 0], [320, 30], [320, 60], [200, 60])],                    # (260, 30): a local extremum ON line 3; (320, 30): a pass-through vertex on it
        [A([400, 0], [520, 0], [520, 60], [460, 30], [400, 60])],                               # (460, 30): the extremum from the other side
        [A([600, 0], [650, 0], [650, 40], [600, 40])],                                          # two sides exactly on lines 0 and 4: the skipped parallel edges
        [sq(700, 0, 90), A([730, 30], [730, 60], [760, 60], [760, 30])],                        # a square with a hole
        [sq(0, 100, 40)], [sq(20, 110, 40)],                                                    # the middle one of three is the unfilled subpath (fill below)
        [sq(50, 130, 40)],
        [A([100, 100], [110, 110], [130, 130])],                                                # collinear along (1, 1): no lines at 45 degrees, degenerate pairs elsewhere
        [sq(200, 100, 30), sq(230, 100, 30)],                                                   # two squares of one group sharing an edge: equal w, twice
        [sq(300, 100, 30), sq(330, 130, 30)],                                                   # ... sharing a vertex
        [A([400, 100], [440, 140], [470, 170], [430, 170])],                                    # vertices on y = x + const: on lines of the 45 degree family
    ]
    fill = [0, 1, 2, 3, 4, 4, 5, -1, 7, 8, 9, 9, 10, 10, 11]
    return [[p + (dx, dy) for p in grp] for grp in g], fill


@pytest.mark.parametrize("angle", sorted(ANGLES))
def test_every_situation_of_the_rule(dev, angle):
    groups, fill = scene()
    u = ANGLES[angle]
    want, st, ks = against_double(dev, groups, 10, 1, u, BOTH, fill=fill)
    assert st["groups"] == 11 and st["segments"] > 100
    against_double(dev, groups, 10, 0, u, HA.HORIZONTAL, fill=fill)                             # no serpentine, no inset: the touching pairs of the shared vertex stay out (we > ws)
    against_double(dev, groups, 7, 2, u, HA.VERTICAL | HA.SERPENTINE, fill=fill)


@pytest.mark.parametrize("angle", [0, 45, 17.5])
def test_negative_coordinates(dev, angle):
    """the scene moved below and left of the origin: negative k, so floor division and the serpentine's k & 1 in two's complement"""
    groups, fill = scene(-450, -130)
    want, st, ks = against_double(dev, groups, 10, 1, ANGLES[angle], BOTH, fill=fill)
    assert (ks < 0).any() and (ks > 0).any() and (ks[ks < 0] & 1).any()


def test_collinear_group_gives_no_lines(dev):
    g = [[A([100, 100], [110, 110], [130, 130])]]
    want, st, _ = against_double(dev, g, 10, 0, (2896, 2896), HA.HORIZONTAL)
    assert st == {"groups": 1, "lines": 0, "crossings": 0, "segments": 0, "collapsed": 0}
    want, st, _ = against_double(dev, g, 10, 0, (2896, 2896), HA.VERTICAL)
    assert st["lines"] > 0 and st["crossings"] == 2 * st["lines"] and st["segments"] == 0      # there and back at the same w


def test_family_order_and_the_flags(dev):
    groups, fill = scene()
    u = ANGLES[30]
    a, ast, _ = against_double(dev, groups, 10, 1, u, HA.HORIZONTAL | HA.SERPENTINE, fill=fill)
    b, bst, _ = against_double(dev, groups, 10, 1, u, HA.VERTICAL | HA.SERPENTINE, fill=fill)
    c, cst, _ = against_double(dev, groups, 10, 1, u, BOTH, fill=fill)
    assert len(a) and len(b) and np.array_equal(c, np.concatenate([a, b]))                      # the family along u first


def test_inset_collapses_segments(dev):
    star = HD.star(np.random.default_rng(0), 0, 0, 60, 9)
    want, st, _ = against_double(dev, [[star]], 4, 3, ANGLES[17.5], BOTH)
    assert st["collapsed"] > 0 and st["segments"] > 0


# ------------------------------------------------------------------ the paths of the kernels
def thin_triangles(n, height=200):
    return [A([12 * i, 0], [12 * i + 8, 3], [12 * i + 4, height]) for i in range(n)]


@pytest.mark.parametrize("n,lo,hi", [(20, 2, 64), (200, 65, 2048), (1100, 2049, 10 ** 9)])
@pytest.mark.parametrize("u", [(4096, 0), (4096, 5)])
def test_rows_of_every_sort_class(dev, n, lo, hi, u):
    """n thin triangles side by side in one group, about 20 lines across all of them: a row holds at most 2 n crossings and, from the double's own kept pairs,
    at least `lo`.  Beside it a small group, so that the wave sort runs in the same call as the block sort"""
    groups = [thin_triangles(n), [A([0, 300], [50, 310], [20, 390])]]
    want, st, ks = against_double(dev, groups, 10, 0, u, HA.HORIZONTAL | HA.SERPENTINE)
    first = ks[:np.count_nonzero(want[:, 1] < 250)]                                             # the lines of the first group
    per_row = 2 * np.bincount(first - first.min()).max()
    assert lo <= per_row and 2 * n <= hi, (per_row, n)
    assert st["lines"] <= 40


def test_mixed_classes_in_one_call(dev):
    groups = [thin_triangles(1100), thin_triangles(200), thin_triangles(20)]
    groups[1] = [p + (0, 400) for p in groups[1]]; groups[2] = [p + (0, 800) for p in groups[2]]
    against_double(dev, groups, 25, 1, (4096, 5), BOTH)


SMALL = [A([0, 300], [50, 310], [20, 390])]                                                     # the second group of the drawings below: rows for the wave sort


def against_plain_double(dev, groups, spacing, inset, flags):
    """orip_svg_hatch on thin_triangles (y < 250) and SMALL (y >= 300) in one direction against the numpy double: the points, the counts, the fetched groups"""
    off, pts, fg = put(dev, groups)
    want, wst = HD.hatch_segments(off, HD.quantise(pts, 1.0), fg, spacing, inset, flags)
    st = dev.svg_hatch(fg, 1.0, spacing, inset, flags)
    assert st == wst, (st, wst)
    o2, p2 = dev.svg_paths()
    assert len(o2) == len(off) + len(want) and np.array_equal(o2[:len(off)], off) and np.array_equal(np.diff(o2[len(off) - 1:]), np.full(len(want), 2))
    assert np.array_equal(p2[:len(pts)], pts) and np.array_equal(p2[len(pts):], want.reshape(-1, 2).astype(np.float64))
    assert np.array_equal(dev.svg_hatch_groups(st["segments"]), np.where(want[:, 1] < 250, 0, 1))
    return want, st


@pytest.mark.parametrize("n", [32, 33, 1024, 1025])
def test_rows_on_the_class_boundaries(dev, n):
    """n thin triangles in one group at spacing 10: every non-empty row of the group holds exactly 2 n crossings = 64 (a full wave, no padding lane), 66 (the
    first row of the block sort), 2048 (a block row with no padding slot), 2050 (the first row that calls the large sort), under both rules"""
    groups = [thin_triangles(n), SMALL]
    small = HD.hatch_segments([0, 3], SMALL[0], [0], 10, 0, HD.HORIZONTAL)[1]
    want, st = against_plain_double(dev, groups, 10, 0, HD.HORIZONTAL)
    # the apex row's pairs have ex == sx and are dropped: 19 rows of n segments, and the crossings say that the twentieth holds 2 n too
    assert st["crossings"] - small["crossings"] == 2 * n * 20 and st["lines"] - small["lines"] == 21 and np.array_equal(np.bincount(want[want[:, 1] < 250, 1] // 10)[1:], np.full(19, n))
    small = HA.hatch_segments_angle([0, 3], SMALL[0], [0], 10, 0, (4096, 0), HA.HORIZONTAL)[1]
    want, st, ks = against_double(dev, groups, 10, 0, (4096, 0), HA.HORIZONTAL)
    # 20 lines, none with more than 2 n crossings (a triangle meets a line twice at most), 2 n * 20 in all: 2 n on each.  The pairs of the two top rows collapse
    assert st["crossings"] - small["crossings"] == 2 * n * 20 and st["lines"] - small["lines"] == 20 and st["collapsed"] - small["collapsed"] == 2 * n


def test_both_rules_alternate_on_one_context():
    """the two rules carve ht_rows and ht_x with records of different sizes and reuse what the last call left: each of four calls on one device equals its
    double, the second pair on a drawing a fifth the size, in buffers the other rule left larger than it needs"""
    from orip.device import Device
    d = Device(0)
    try:
        for n in (200, 40):
            groups = [thin_triangles(n), SMALL]
            want, st = against_plain_double(d, groups, 10, 1, HD.HORIZONTAL | HD.SERPENTINE)
            assert st["segments"] > 10 * n
            want, st, _ = against_double(d, groups, 10, 1, ANGLES[30], BOTH)
            assert st["segments"] > 10 * n
    finally:
        d.close()


def test_edges_of_many_chunks(dev):
    tall = A([0, 0], [300, 1000], [-200, 700])
    want, st, _ = against_double(dev, [[tall]], 3, 1, ANGLES[17.5], BOTH)
    assert st["lines"] > 2 * 64 * 3 and st["crossings"] > 600                                   # each long edge crosses several chunks of 64 lines


def test_widest_products(dev):
    m = 2 ** 24 - 1
    tri = A([-m, -m], [m, -m + 5], [3, m])
    want, st, _ = against_double(dev, [[tri]], 2 ** 20, 1000, (3547, 2048), BOTH)
    assert st["segments"] > 20
    against_double(dev, [[tri]], 2 ** 20, 1000, (-4096, 4095), BOTH)
    against_double(dev, [[tri]], 2 ** 31 - 1, 2 ** 31 - 1, (4096, 4096), BOTH)                  # the largest D and I: no lines inside, nothing overflows


def test_quantisation_and_steps_per_mm(dev):
    """coordinates that are not whole steps, ties among them: q = rint(v * spm), and the lines come back as round4(k / spm), which names every step"""
    rng = np.random.default_rng(17)
    shapes = [[HD.star(rng, int(rng.integers(0, 2000)), int(rng.integers(0, 2000)), int(rng.integers(20, 150)), int(rng.integers(3, 12)))] for _ in range(25)]
    for spm in (40.0, 7.3, 5000.0):
        t = HD.polys_table([[p / spm + rng.choice([0.0, 0.5 / spm, 0.0125, 1e-4], p.shape) for p in g] for g in shapes])
        dev.svg_flatten(t, 1.0); dev.svg_fit(1.0, 1.0, 0.0, 0.0)
        off, pts = dev.svg_paths()
        want, wst = HA.hatch_segments_angle(off, HA.quantise(pts, spm), t.fill_group, 20, 3, ANGLES[30], BOTH)
        assert dev.svg_hatch_angle(t.fill_group, spm, 20, 3, ANGLES[30], BOTH) == wst and wst["segments"] > 100
        o2, p2 = dev.svg_paths()
        mm = round4_python(want.reshape(-1, 2).astype(np.float64) / spm)
        assert np.array_equal(p2[len(pts):], mm) and np.array_equal(np.rint(mm * spm).astype(np.int64), want.reshape(-1, 2))


# ------------------------------------------------------------------ error returns
def test_error_returns_leave_nothing_behind(dev):
    from orip.device import OripError
    ring = [A([0, 0], [400, 0], [400, 400], [0, 400]), A([150, 150], [150, 250], [250, 250], [250, 150])]
    u, F = ANGLES[30], HA.HORIZONTAL | HA.SERPENTINE
    dev.svg_flatten(HD.polys_table([ring]), 1.0)
    with pytest.raises(OripError):                                                              # flattened, not fitted
        dev.svg_hatch_angle([0, 0], 1.0, 20, 3, u, F)
    off, pts, fg = put(dev, [ring])
    before = dev.svg_paths()

    def refused(*a):
        with pytest.raises(OripError):
            dev.svg_hatch_angle(*a)
        after = dev.svg_paths()
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    refused([0, 0, 0], 1.0, 20, 3, u, F); refused([0], 1.0, 20, 3, u, F)                        # not the resident count
    refused([0, 2], 1.0, 20, 3, u, F); refused([-2, 0], 1.0, 20, 3, u, F)                       # group out of range
    refused(fg, 1.0, 0, 3, u, F); refused(fg, 1.0, 20, -1, u, F)
    refused(fg, 1.0, 20, 3, u, HA.SERPENTINE); refused(fg, 1.0, 20, 3, u, 8 | F)
    for bad in ((0, 0), (4097, 0), (0, -4097), (-4097, 4096), (2 ** 31 - 1, 1)):                # u out of range
        refused(fg, 1.0, 20, 3, bad, F)
    for spm in (0.0, -1.0, 5000.5, np.inf, np.nan):
        refused(fg, spm, 20, 3, u, F)
    want, wst = HA.hatch_segments_angle(off, pts, fg, 20, 3, u, F)
    assert dev.svg_hatch_angle(fg, 1.0, 20, 3, u, F) == wst and wst["segments"] > 10            # and then it works
    hatched = dev.svg_paths()
    assert np.array_equal(hatched[1][len(pts):].reshape(-1, 4), want)
    for again in (lambda: dev.svg_hatch_angle(fg, 1.0, 20, 3, u, F), lambda: dev.svg_hatch(fg, 1.0, 20, 3, F)):      # a second hatch of either kind
        with pytest.raises(OripError):
            again()
        assert np.array_equal(dev.svg_paths()[1], hatched[1])
    off, pts, fg = put(dev, [ring])
    dev.svg_hatch(fg, 1.0, 20, 3, F)
    hatched = dev.svg_paths()
    with pytest.raises(OripError):                                                              # and the new one behind the old one
        dev.svg_hatch_angle(fg, 1.0, 20, 3, u, F)
    assert np.array_equal(dev.svg_paths()[1], hatched[1])

    def big(polys, spm, spacing, flags=HA.HORIZONTAL, uu=(4096, 0)):
        off, pts, fg = put(dev, [polys])
        with pytest.raises(OripError):
            dev.svg_hatch_angle(fg, spm, spacing, 0, uu, flags)
        after = dev.svg_paths()
        assert np.array_equal(after[0], off) and np.array_equal(after[1], pts)
    big([A([0, 0], [2 ** 24, 0], [5, 9])], 1.0, 3)                                              # |q| = 2^24
    big([A([0, 0], [-2 ** 24, 0], [5, 9])], 1.0, 3, uu=u)
    big([A([0, 0], [1000, 0], [500, 4000])], 5000.0, 3)                                         # 2e7 steps
    with pytest.raises(ValueError):
        HA.quantise(A([0, 0], [2 ** 24, 0], [5, 9]), 1.0)
    off, pts, _ = put(dev, [ring])
    assert dev.svg_hatch_angle([-1, -1], 1.0, 20, 3, u, F) == {"groups": 0, "lines": 0, "crossings": 0, "segments": 0, "collapsed": 0}
    assert np.array_equal(dev.svg_paths()[1], pts)


def test_a_failing_second_family_appends_nothing(dev):
    """20 tall triangles, u = (0, 1), spacing 1: along u the lines are x = const, a thousand of them; across u they are y = const, 2^25 lines that every long
    edge crosses -- 20 * 2^26 crossings, beyond the cap of 2^30.  The call fails behind the first family's kernels and leaves the paths alone.  (The cap of
    2^26 lines cannot be reached below 2^24 steps: at most 2^26 - 4 lines lie across a drawing, at u = (1, 1).)"""
    from orip.device import OripError
    m = 2 ** 24 - 1
    tris = [A([k, -m], [1000 - k, -m], [500, m]) for k in range(20)]
    off, pts, fg = put(dev, [tris])
    for flags in (HA.HORIZONTAL | HA.VERTICAL, HA.VERTICAL):
        with pytest.raises(OripError, match="crossings"):
            dev.svg_hatch_angle(fg, 1.0, 1, 0, (0, 1), flags)
        after = dev.svg_paths()
        assert np.array_equal(after[0], off) and np.array_equal(after[1], pts)
    want, wst = HA.hatch_segments_angle(off, pts, fg, 1, 0, (0, 1), HA.HORIZONTAL)              # the same paths, the family that fits
    assert dev.svg_hatch_angle(fg, 1.0, 1, 0, (0, 1), HA.HORIZONTAL) == wst and wst["lines"] == 1000
    assert np.array_equal(dev.svg_paths()[1][len(pts):].reshape(-1, 4), want)


# ------------------------------------------------------------------ the resident hand-off
def test_resident_hand_off(dev):
    from orip.device import OripError
    ring = [A([0, 0], [400, 0], [400, 400], [0, 400]), A([150, 150], [150, 250], [250, 250], [250, 150])]
    off, pts, fg = put(dev, [ring])
    want, wst = HA.hatch_segments_angle(off, pts, fg, 20, 3, ANGLES[-60], BOTH)
    assert dev.svg_hatch_angle(fg, 1.0, 20, 3, ANGLES[-60], BOTH) == wst
    o2, p2 = dev.svg_paths()
    with pytest.raises(OripError):
        dev.gcode_to_steps(None, None, STEP_MAP, n=2)                                           # the count is the hatched one now
    soff, spts = dev.gcode_to_steps(None, None, STEP_MAP, n=len(o2) - 1)
    assert np.array_equal(spts[soff[len(soff) - 1 - len(want)]:].reshape(-1, 4), want)
    b = dev.gcode_to_steps(o2, p2, STEP_MAP)
    assert np.array_equal(b[0], soff) and np.array_equal(b[1], spts)


# ------------------------------------------------------------------ the whole tool
HATCH = ["--hatch-spacing-mm", "5", "--hatch-inset-mm", "0.5", "--hatch-angle-deg", "30", "--hatch-direction", "cross"]


def tool_doubles():
    import clip_double as CD
    import dedup_double as DD
    import occlude_cases as OC
    H = HA.HatchAngleWithGroups()
    return dict(CD.svg_doubles(), dedup_fn=DD.dedup_numpy, occlude_fn=OC.OccludeDouble(), hatch_fn=H.hatch, hatch_groups_fn=H.hatch_groups)


def svg_options(args):
    from orip import svg as SV
    return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + list(args)))


@pytest.mark.parametrize("extra", [[], ["--pen-colors", "#ccc,#f00,#00f"], ["--occlude"]], ids=["plain", "pens", "occlude"])
def test_tool_in_process_matches_the_doubles(dev, extra):
    from orip import svg as SV
    import occlude_cases as OC
    o = svg_options(["--scale", "1", "--margin-mm", "0", "--steps-per-mm", "4"] + HATCH + extra)
    want, winfo = SV.build_stream_from_svg(OC.TOOL_SVG, o, want_paths=True, **tool_doubles())
    got, info = SV.build_stream_from_svg(OC.TOOL_SVG, o, dev, want_paths=True)
    assert info["hatch"] == winfo["hatch"] and info["hatch"]["segments"] > 20 and "collapsed" in info["hatch"] and info["hatch_u"] == (3547, 2048)
    assert np.array_equal(info["fitted_paths"][0], winfo["fitted_paths"][0]) and np.array_equal(info["fitted_paths"][1], winfo["fitted_paths"][1])
    assert got == want
    if extra == ["--pen-colors", "#ccc,#f00,#00f"]:
        assert np.array_equal(info["path_pens"], winfo["path_pens"]) and len(set(np.asarray(info["path_pens"])[-info["hatch"]["segments"]:].tolist())) > 1
    if extra == ["--occlude"]:
        assert info["occlude"] == winfo["occlude"] and info["occlude"]["cut"] > 0
    assert SV.build_stream_from_svg(OC.TOOL_SVG, o, dev)[0] == want                             # the points never fetched


def test_scripts_on_disk(tmp_path):
    from orip import svg as SV
    import occlude_cases as OC
    args = ["--scale", "1", "--margin-mm", "0", "--steps-per-mm", "4"] + HATCH
    want, winfo = SV.build_stream_from_svg(OC.TOOL_SVG, svg_options(args), want_paths=True, **tool_doubles())
    text = SV.gcode_text(*winfo["fitted_paths"])
    src = tmp_path / "drawing.svg"; src.write_bytes(OC.TOOL_SVG)
    run = lambda script, extra: subprocess.run([sys.executable, os.path.join(SCRIPTS, script), str(src)] + extra, capture_output=True, text=True, timeout=300)
    r = run("svg2stream.py", ["--no-preview"] + args)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "drawing_stream.bin").read_bytes() == want and (tmp_path / "drawing.gcode").read_text() == text
    report = "%d collapsed, at %.4f deg (u = (3547, 2048))" % (winfo["hatch"]["collapsed"], SV.hatch_effective_angle((3547, 2048)))
    assert "[svg] hatch: %d fill groups" % winfo["hatch"]["groups"] in r.stdout and report in r.stdout
    r = run("svg2gcode.py", ["-o", str(tmp_path / "h.gcode")] + args)
    assert r.returncode == 0 and (tmp_path / "h.gcode").read_text() == text and report in r.stdout
    r = run("svg2stream.py", ["-o", str(tmp_path / "bad.bin"), "--gcode-output", str(tmp_path / "bad.gcode"), "--no-preview", "--hatch-spacing-mm", "1", "--hatch-angle-deg", "nan"])
    assert r.returncode != 0 and not (tmp_path / "bad.bin").exists() and not (tmp_path / "bad.gcode").exists()


def test_preview_shows_the_filled_ring(dev):
    """a 400-step square with a 100-step hole, crossed at +-45 degrees every 4 steps with no inset: no ink in the hole's interior, and ink in every 16 x 16 tile
    well inside the ring -- a tile's extent along n is at least 16 > 4, so a line passes through it"""
    from orip import svg as SV, stream_preview as SP
    from test_svg_host import options_for
    from test_hatch_host import svg_of
    ring = [A([0, 0], [400, 0], [400, 400], [0, 400]), A([150, 150], [150, 250], [250, 250], [250, 150])]
    args = ["--scale", "0.025", "--margin-mm", "0", "--page-width-mm", "10", "--page-height-mm", "10", "--hatch-spacing-mm", "0.1", "--hatch-inset-mm", "0", "--hatch-direction", "cross",
            "--hatch-angle-deg", "45"]
    data, info = SV.build_stream_from_svg(svg_of(ring), options_for(args), dev)
    # about 141 lines per family cross the square (800 * 2896 / D, D = 16382), each with a segment or two: more than 270 in all
    assert tuple(info["target"]) == (400, 400) and info["hatch"]["segments"] > 270 and info["hatch_u"] == (2896, 2896)
    rgb, st = SP.preview(dev, data, 400, 400, 400, 400, invert_y=True)
    ink = (rgb != 255).any(2)
    assert st["off_canvas_draws"] == 0 and not ink[160:240, 160:240].any()
    tiles = ink[16:384, 16:384].reshape(23, 16, 23, 16).any(axis=(1, 3))
    inside_hole = np.zeros((23, 23), bool); inside_hole[8:15, 8:15] = True                      # the tiles that touch [144, 256): the hole and its rim
    assert tiles[~inside_hole].all()
