"""The hatch at an angle on the CPU: the sequential double (tests/hatch_angle_double.py) held to the properties the rule promises -- it agrees with the
reference's rule where the two must agree, it is covariant under the translations of its own line family, every segment lies on its line, and it covers
the area -- and the option's way through orip/svg.py: parsing, the reduction of the angle, the routing on "u", the report."""
import math

import numpy as np
import pytest

import hatch_double as HD
import hatch_angle_double as HA
import svg_double as SD

ANGLES = {0: (4096, 0), 90: (0, 4096), 45: (2896, 2896), 30: (3547, 2048), -60: (2048, -3547), 17.5: (3906, 1232)}


def offsets(polys):
    return np.concatenate([[0], np.cumsum([len(p) for p in polys])])


def undirected(seg):
    s = np.asarray(seg, np.int64).reshape(-1, 4)
    flip = (s[:, 0] > s[:, 2]) | ((s[:, 0] == s[:, 2]) & (s[:, 1] > s[:, 3]))
    s = np.where(flip[:, None], s[:, [2, 3, 0, 1]], s)
    return sorted(map(tuple, s.tolist()))


def test_rs_is_the_nearest_integer_to_the_root():
    for v in list(range(0, 200)) + [2 ** 87 - 1, 2 ** 62 * 33554432, 12345678901234567890123]:
        r = HA.rs(v)
        assert (r == 0 or (2 * r - 1) ** 2 <= 4 * v) and 4 * v < (2 * r + 1) ** 2            # r - 1/2 <= sqrt(v) < r + 1/2
    assert HA.rs(20 * 20 * 4096 * 4096) == 20 * 4096


def test_rectangles_at_angle_zero_draw_what_the_reference_rule_draws():
    """integer rectangles, u = (4096, 0): s = 4096 y, D = 4096 spacing, so the lines are the multiples of the spacing -- the reference's own lines, whose
    anchor y0 is a multiple too; every crossing is an integer x, so truncation and rounding agree.  Undirected: the two count serpentine parity differently"""
    rng = np.random.default_rng(1)
    for trial in range(40):
        n = int(rng.integers(1, 4))
        polys = []
        for _ in range(n):
            x0, y0 = rng.integers(-300, 300, 2); w, h = rng.integers(1, 200, 2)
            polys.append(np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]], np.int64))
        gid = rng.integers(0, n, n)
        spacing, inset = int(rng.integers(1, 30)), int(rng.integers(0, 6))
        off, q = offsets(polys), np.concatenate(polys)
        want, _ = HD.hatch_segments(off, q, gid, spacing, inset, HD.HORIZONTAL)
        got, st = HA.hatch_segments_angle(off, q, gid, spacing, inset, (4096, 0), HA.HORIZONTAL)
        assert undirected(got) == undirected(want) and st["collapsed"] == 0


def drawing(seed, groups=6):
    rng = np.random.default_rng(seed)
    polys, gid = [], []
    for g in range(groups):
        for _ in range(int(rng.integers(1, 3))):
            polys.append(HD.star(rng, int(rng.integers(-500, 500)), int(rng.integers(-500, 500)), int(rng.integers(20, 200)), int(rng.integers(3, 12))))
            gid.append(g)
    return polys, np.asarray(gid)


@pytest.mark.parametrize("angle", sorted(ANGLES))
def test_translation_along_the_family_moves_every_coordinate(angle):
    u = ANGLES[angle]
    g = math.gcd(*u)
    step = np.array([u[0] // g, u[1] // g], np.int64)
    polys, gid = drawing(int(angle * 2) + 200)
    off, q = offsets(polys), np.concatenate(polys)
    F = HA.HORIZONTAL | HA.SERPENTINE
    base, bst = HA.hatch_segments_angle(off, q, gid, 13, 2, u, F)
    assert len(base) > 20
    for m in (1, -3):
        moved, mst = HA.hatch_segments_angle(off, q + m * step, gid, 13, 2, u, F)
        assert mst == bst and np.array_equal(moved, base + np.tile(m * step, 2))


@pytest.mark.parametrize("angle", sorted(ANGLES))
def test_both_ends_lie_within_half_a_step_of_their_line(angle):
    """rounding moves a coordinate by at most 1/2, so n . p by at most (|ux| + |uy|) / 2 -- for both ends, for the SAME k"""
    u = ANGLES[angle]
    polys, gid = drawing(int(angle * 2) + 300)
    seg, st, grp, ks, us = HA.hatch_lines_angle(offsets(polys), np.concatenate(polys), gid, 9, 1, u, HA.HORIZONTAL | HA.VERTICAL | HA.SERPENTINE)
    assert len(seg) > 100 and (np.diff(grp[:np.argmax((us != us[0]).any(1))]) >= 0).all()
    D = HA.rs(81 * (u[0] ** 2 + u[1] ** 2))
    for (x0, y0, x1, y1), k, (fx, fy) in zip(seg.tolist(), ks.tolist(), us.tolist()):
        for x, y in ((x0, y0), (x1, y1)):
            assert 2 * abs(-fy * x + fx * y - k * D) <= abs(fx) + abs(fy)


def convex(rng, r):
    """a convex polygon of integer vertices: the hull of random points"""
    p = np.unique(np.rint(rng.normal(0, r, (40, 2))).astype(np.int64), axis=0)
    p = p[np.lexsort((p[:, 1], p[:, 0]))]
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for pt in p.tolist():
        while len(lower) >= 2 and cross(lower[-2], lower[-1], pt) <= 0: lower.pop()
        lower.append(pt)
    for pt in reversed(p.tolist()):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], pt) <= 0: upper.pop()
        upper.append(pt)
    return np.asarray(lower[:-1] + upper[:-1], np.int64)


@pytest.mark.parametrize("angle", sorted(ANGLES))
@pytest.mark.parametrize("spacing", [1, 7])
def test_convex_area_is_covered(angle, spacing):
    """Inset 0, a convex polygon: sum(length) * spacing is within perimeter * spacing + 2 * segments of the area, at every spacing.  Why that margin holds:
    the chord length c(t) across the direction is concave on its support, so unimodal, with maximum M <= perimeter / 2 (a chord is no longer than either arc
    of the outline between its ends), and its total variation over the real line is 2 M.  Give every line the cell of width d = D / |u| around it: inside a
    cell c differs from its value on the line by at most the variation of the half cell, so sum c(k d) d misses the integral, the area, by at most
    d * (2 M) / 2 = d M <= d * perimeter / 2.  Rounding moves each end of a segment by at most sqrt(2) / 2, so a drawn length is off by at most sqrt(2), and
    a collapsed segment (dropped) was at most sqrt(2) long: spacing * sqrt(2) * (segments + collapsed).  d is the spacing within 1 / (2 |u|), which adds
    sum(length) / (2 |u|).  Together the SHARP margin spacing * (perimeter / 2 + sqrt(2) * (segments + collapsed)) + sum(length) / (2 |u|).  A convex polygon
    has one segment per line and its extent across the lines is at most perimeter / 2, so segments + collapsed <= perimeter / (2 d) + 1 and the rounding term
    is about 0.71 * perimeter: from spacing 2 on it fits into the other half of perimeter * spacing, and at spacing 1, where a length and a length times the
    spacing are one unit, sqrt(2) < 2 carries it.  The test asserts the margin as stated, the sharp one, and that the sharp one lies inside the stated one."""
    u = ANGLES[angle]
    P = convex(np.random.default_rng(int(angle * 2) + 400 + spacing), 150)
    x, y = P[:, 0].astype(float), P[:, 1].astype(float)
    area = 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))
    perimeter = np.hypot(*(P - np.roll(P, -1, 0)).T.astype(float)).sum()
    seg, st = HA.hatch_segments_angle([0, len(P)], P, [0], spacing, 0, u, HA.HORIZONTAL)
    length = np.hypot(seg[:, 2] - seg[:, 0], seg[:, 3] - seg[:, 1]).sum()
    stated = perimeter * spacing + 2 * st["segments"]
    sharp = spacing * (perimeter / 2 + math.sqrt(2) * (st["segments"] + st["collapsed"])) + length / (2 * math.hypot(*u))
    assert area > 20000 and st["segments"] > 20
    assert abs(length * spacing - area) <= stated, (length * spacing, area, stated)
    assert abs(length * spacing - area) <= sharp <= stated, (length * spacing, area, sharp, stated)


def test_order_families_groups_and_refusals():
    polys, gid = drawing(7, groups=3)
    off, q = offsets(polys), np.concatenate(polys)
    u = ANGLES[30]
    a, ast = HA.hatch_segments_angle(off, q, gid, 11, 1, u, HA.HORIZONTAL | HA.SERPENTINE)
    b, bst = HA.hatch_segments_angle(off, q, gid, 11, 1, u, HA.VERTICAL | HA.SERPENTINE)
    c, cst = HA.hatch_segments_angle(off, q, gid, 11, 1, u, HA.HORIZONTAL | HA.VERTICAL | HA.SERPENTINE)
    assert len(a) and len(b) and np.array_equal(c, np.concatenate([a, b])) and all(cst[k] == ast[k] + bst[k] for k in ("lines", "crossings", "segments", "collapsed"))
    b2, _ = HA.hatch_segments_angle(off, q, gid, 11, 1, (-u[1], u[0]), HA.HORIZONTAL | HA.SERPENTINE)
    assert np.array_equal(b, b2)                                           # "across u" is "along (-uy, ux)"
    # the caller's group numbers decide the order, not the order of the subpaths
    swapped = np.where(gid == 0, 2, np.where(gid == 2, 0, gid))
    s, _, sg, _, _ = HA.hatch_lines_angle(off, q, swapped, 11, 1, u, HA.HORIZONTAL)
    assert (np.diff(sg) >= 0).all() and set(sg.tolist()) == {0, 1, 2}
    for bad in (dict(u=(0, 0)), dict(u=(4097, 0)), dict(u=(0, -4097)), dict(spacing=0), dict(inset=-1), dict(flags=HA.SERPENTINE), dict(flags=8 | HA.HORIZONTAL)):
        k = dict(dict(u=u, spacing=11, inset=1, flags=HA.HORIZONTAL), **bad)
        with pytest.raises(ValueError):
            HA.hatch_segments_angle(off, q, gid, k["spacing"], k["inset"], k["u"], k["flags"])
    with pytest.raises(ValueError):
        HA.hatch_segments_angle([0, 3], [[0, 0], [2 ** 24, 0], [0, 5]], [0], 1, 0, u, HA.HORIZONTAL)
    with pytest.raises(ValueError):
        HA.quantise(np.array([[2.0 ** 24, 0.0]]), 1.0)


def test_widest_products_triangle():
    """corners at +-(2^24 - 1): the double itself has no width to overflow, so this pins the answer the device must reach"""
    m = 2 ** 24 - 1
    tri = np.array([[-m, -m], [m, -m + 5], [3, m]], np.int64)
    seg, st = HA.hatch_segments_angle([0, 3], tri, [0], 2 ** 20, 1000, (3547, 2048), HA.HORIZONTAL | HA.VERTICAL | HA.SERPENTINE)
    assert st["segments"] == len(seg) > 20 and st["crossings"] == 2 * st["lines"] and np.abs(seg).max() < 2 ** 24


# ------------------------------------------------------------------ the option
def test_option_parsing_and_the_reduction_of_the_angle():
    from orip import svg as SV
    from test_svg_host import options_for
    assert SV.SvgOptions().hatch_angle_deg is None
    old = {"spacing": 20, "inset": 27, "flags": HD.HORIZONTAL | HD.SERPENTINE, "steps_per_mm": 40.0}
    assert SV.hatch_params(options_for(["--hatch-spacing-mm", "0.5"])) == old                          # without the option: the dict as it was
    assert SV.hatch_params(options_for(["--hatch-angle-deg", "45"])) is None                           # without a spacing the angle is ignored, as the inset is
    assert SV.hatch_params(options_for(["--hatch-angle-deg", "nan"])) is None
    assert SV.hatch_params(options_for(["--hatch-spacing-mm", "0.5", "--hatch-angle-deg", "45"])) == dict(old, u=(2896, 2896))
    for a, u in list(ANGLES.items()) + [(135, (2896, -2896)), (-90, (0, 4096)), (180, (4096, 0)), (-135, (2896, 2896)), (450, (0, 4096)), (-45, (2896, -2896)), (89.99, (1, 4096))]:
        assert SV.hatch_direction_vector(a) == u, a
    for bad in ("nan", "inf", "-inf"):
        with pytest.raises(ValueError):
            SV.hatch_params(options_for(["--hatch-spacing-mm", "0.5", "--hatch-angle-deg=" + bad]))
    p = SV.hatch_params(options_for(["--hatch-spacing-mm", "1", "--hatch-angle-deg", "30", "--hatch-direction", "cross", "--no-serpentine"]))
    assert p["flags"] == HD.HORIZONTAL | HD.VERTICAL and p["u"] == (3547, 2048)
    g = SV.options_from_args(SV.build_gcode_argparser().parse_args(["x.svg", "--hatch-spacing-mm", "2", "--hatch-angle-deg", "-60"]))
    assert g.hatch_angle_deg == -60.0
    assert abs(SV.hatch_effective_angle((2896, 2896)) - 45.0) < 1e-12 and abs(SV.hatch_effective_angle((3906, 1232)) - 17.5) < 0.01


def test_resident_routes_on_u():
    from orip import svg as SV

    class Dev:
        def __init__(self): self.calls = []
        def svg_hatch(self, *a): self.calls.append(("plain", a)); return {"groups": 1, "lines": 2, "crossings": 4, "segments": 2}
        def svg_hatch_angle(self, *a): self.calls.append(("angle", a)); return {"groups": 1, "lines": 2, "crossings": 4, "segments": 1, "collapsed": 1}
    d = Dev()
    r = SV._Resident(d)
    prm = {"spacing": 20, "inset": 3, "flags": 3, "steps_per_mm": 40.0}
    assert r.hatch({"n": 1, "total": 4}, [0], prm)[0] == {"n": 3, "total": 8}
    assert r.hatch({"n": 1, "total": 4}, [0], dict(prm, u=(2896, 2896)))[0] == {"n": 2, "total": 6}
    assert d.calls == [("plain", ([0], 40.0, 20, 3, 3)), ("angle", ([0], 40.0, 20, 3, (2896, 2896), 3))]


def test_tool_on_the_doubles_and_the_report(tmp_path, capsys):
    """the whole tool with every device step on the CPU: the slanted lines reach the step paths, the G-code and the report; without the option nothing moves"""
    from orip import svg as SV, gcode as GC
    from test_svg_host import options_for
    from test_hatch_host import svg_of, TOOL
    ring = [np.array([[0, 0], [400, 0], [400, 400], [0, 400]], np.int64), np.array([[150, 150], [150, 250], [250, 250], [250, 150]], np.int64)]
    args = TOOL + ["--hatch-spacing-mm", "0.5", "--hatch-inset-mm", "0.05", "--hatch-angle-deg", "30", "--hatch-direction", "cross"]
    H = HA.HatchAngleWithGroups()
    data, info = SV.build_stream_from_svg(svg_of(ring), options_for(args), want_paths=True, **dict(SD.svg_doubles(), hatch_fn=H.hatch, hatch_groups_fn=H.hatch_groups))
    off, pts = info["fitted_paths"]
    q = HA.quantise(pts[:off[2]], 40.0)
    want, wst = HA.hatch_segments_angle(off[:3], q, [0, 0], 20, 2, (3547, 2048), HA.HORIZONTAL | HA.VERTICAL | HA.SERPENTINE)
    assert info["hatch"] == wst and set(info["hatch"]) == {"groups", "lines", "crossings", "segments", "collapsed"} and info["hatch_u"] == (3547, 2048) and len(want) > 20
    assert np.array_equal(np.rint(pts[off[2]:] * 40.0).astype(np.int64).reshape(-1, 4), want)
    plain, pinfo = SV.build_stream_from_svg(svg_of(ring), options_for(TOOL + ["--hatch-spacing-mm", "0.5", "--hatch-inset-mm", "0.05", "--hatch-direction", "cross"]),
                                            **dict(SD.svg_doubles(), hatch_fn=HD.hatch_numpy))
    assert set(pinfo["hatch"]) == {"groups", "lines", "crossings", "segments"} and "hatch_u" not in pinfo and plain != data
    src = tmp_path / "d.svg"; src.write_text(svg_of(ring))
    R = dict(flatten_fn=SD.flatten_numpy, bbox_fn=SD.bbox_numpy, fit_fn=SD.fit_numpy, fetch_fn=SD.fetch_numpy, hatch_fn=HA.hatch_angle_numpy)
    SV.main_gcode([str(src), "-o", str(tmp_path / "d.gcode")] + args[:4] + args[5:], **R)
    goff, gpts, _ = GC.parse_gcode((tmp_path / "d.gcode").read_text())
    assert np.array_equal(np.rint(gpts[goff[2]:] * 40.0).astype(np.int64).reshape(-1, 4), want)
    out = capsys.readouterr().out
    assert "at %.4f deg (u = (3547, 2048))" % math.degrees(math.atan2(2048, 3547)) in out and "at 30.00" in out and "%d collapsed" % wst["collapsed"] in out
