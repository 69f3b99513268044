"""The hatch fill on the CPU: the numpy double (tests/hatch_double.py) against every call the reference's hatch_fill made (tests/golden/golden_hatch.npz,
make_golden_hatch.py), the fill groups parse_svg assigns, the options, and the whole tool with every device step replaced by its double: untouched without
the options, the reference's integers in the step paths with them.  Every comparison is equality."""
import json

import numpy as np
import pytest

from util import load
import hatch_double as HD
import svg_double as SD
import gcode_double as GD

H = load("golden_hatch.npz")
CASES = json.loads(bytes(H["names"]).decode())
NS = 'xmlns="http://www.w3.org/2000/svg"'


def case(name):
    off, pts = H[f"{name}_off"].astype(np.int64), H[f"{name}_pts"].astype(np.int64)
    spacing, inset, serp = (int(v) for v in H[f"{name}_prm"])
    return [pts[a:b] for a, b in zip(off[:-1], off[1:])], spacing, inset, bool(serp), H[f"{name}_seg"].astype(np.int64)


def flags_of(serp, direction=HD.HORIZONTAL):
    return direction | (HD.SERPENTINE if serp else 0)


# ------------------------------------------------------------------ the double against the reference
def test_fixture_holds_the_designed_cases():
    want = {"hole", "nested_overlapping", "horizontal_edges_on_lines", "vertices_on_lines", "negative_coordinates", "inset_swallows", "lower_than_spacing", "between_lines_empty",
            "islands_empty_lines", "comb_block", "comb_segmented"}
    assert want <= set(CASES) and sum(n.startswith("random_") for n in CASES) >= 60
    per_row = lambda n: np.bincount(case(n)[4][:, 1] - case(n)[4][:, 1].min()).max()
    assert 64 < 2 * per_row("comb_block") <= 2048 < 2 * per_row("comb_segmented")        # crossings per row: the block sort, and beyond it
    assert {int(H[f"{n}_prm"][0]) for n in CASES} >= {1, 7, 20, 40, 333} and {int(H[f"{n}_prm"][1]) for n in CASES} >= {0, 3, 27}
    assert {int(H[f"{n}_prm"][2]) for n in CASES} == {0, 1}
    assert all(len(H[f"{n}_seg"]) > 0 for n in CASES if n not in ("between_lines_empty", "two_points"))


@pytest.mark.parametrize("name", CASES)
def test_double_equals_reference(name):
    polys, spacing, inset, serp, want = case(name)
    off = np.concatenate([[0], np.cumsum([len(p) for p in polys])])
    got, st = HD.hatch_segments(off, np.concatenate(polys), np.zeros(len(polys), np.int64), spacing, inset, flags_of(serp))
    assert np.array_equal(got, want) and st["segments"] == len(want) and st["groups"] == 1


def test_double_groups_directions_and_refusals():
    a, b = case("hole"), case("islands_empty_lines")
    polys = a[0] + b[0]
    off = np.concatenate([[0], np.cumsum([len(p) for p in polys])])
    gid = np.array([4] * len(a[0]) + [2] * len(b[0]))                                    # group 2 goes first although its subpaths come last
    got, st = HD.hatch_segments(off, np.concatenate(polys), gid, 20, 3, flags_of(True))
    assert a[1:4] == b[1:4] == (20, 3, True) and np.array_equal(got, np.concatenate([b[4], a[4]])) and st["groups"] == 2
    q = np.concatenate(a[0])
    h, _ = HD.hatch_segments(off[:3], q, [0, 0], 20, 3, flags_of(True))
    v, _ = HD.hatch_segments(off[:3], q[:, ::-1], [0, 0], 20, 3, flags_of(True, HD.VERTICAL))
    assert len(h) and np.array_equal(v, h[:, [1, 0, 3, 2]])                               # vertical = horizontal of the transposed drawing, swapped back
    c, st = HD.hatch_segments(off[:3], q, [0, 0], 20, 3, flags_of(True, HD.HORIZONTAL | HD.VERTICAL))
    v2, _ = HD.hatch_segments(off[:3], q, [0, 0], 20, 3, flags_of(True, HD.VERTICAL))
    assert np.array_equal(c, np.concatenate([h, v2])) and st["segments"] == len(h) + len(v2)
    assert len(HD.hatch_segments(off[:3], q, [-1, -1], 20, 3, flags_of(True))[0]) == 0
    for bad in (dict(spacing=0), dict(inset=-1), dict(flags=HD.SERPENTINE), dict(gid=[0, 2])):
        k = dict(dict(gid=[0, 0], spacing=20, inset=3, flags=flags_of(True)), **bad)
        with pytest.raises(ValueError):
            HD.hatch_segments(off[:3], q, k["gid"], k["spacing"], k["inset"], k["flags"])
    with pytest.raises(ValueError):
        HD.quantise(np.array([[2.0 ** 30, 0.0]]), 1.0)
    assert HD.quantise(np.array([[0.5, 1.5], [2.5, -0.5]]), 1.0).tolist() == [[0, 2], [2, 0]]   # ties to even


# ------------------------------------------------------------------ the fill groups of parse_svg
FILLS = f'''<svg {NS} width="100" height="100">
  <rect width="10" height="10"/>
  <rect width="10" height="10" fill="red"/>
  <rect width="10" height="10" style="stroke:#000;fill:#00f"/>
  <rect width="10" height="10" fill="none"/>
  <rect width="10" height="10" fill="red" style="fill:none"/>
  <g fill="green"><circle r="5"/><g><ellipse rx="3" ry="2"/><polygon points="0,0 5,0 5,5" fill="none"/><polyline points="0,0 5,0 5,5" style="fill: transparent "/></g>
    <line x1="0" y1="0" x2="9" y2="9"/><path d="M0 0L9 0 9 9zM2 1L8 1 8 7zM20 20L30 20 30 30"/></g>
  <g style="fill:none"><rect width="4" height="4"/><rect width="4" height="4" fill="#123"/></g>
  <rect width="0" height="4" fill="red"/>
  <path d="M0 0Q5 5 9 0" fill="black"/>
</svg>'''


def test_parse_svg_fill_groups():
    from orip.svg import parse_svg, SegmentTable
    t = parse_svg(FILLS)
    #        rect, red, style, none, style-over-attribute, circle, ellipse, polygon none, polyline transparent, line, path (3 subpaths), g none: rect, rect own, (empty rect), path
    want = [-1, 1, 2, -1, -1, 5, 6, -1, -1, -1, 10, 10, 10, -1, 12, 13]
    assert t.fill_group.tolist() == want and t.fill_group.dtype == np.int32 and len(want) == t.n_sub
    a = parse_svg(FILLS, "all")
    assert a.fill_group.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, -1, 10, 10, 10, 11, 12, 13]                                  # every element that draws, except the line
    assert np.array_equal(a.kind, t.kind) and np.array_equal(a.ctrl, t.ctrl) and np.array_equal(a.sub_off, t.sub_off)
    with pytest.raises(ValueError):
        parse_svg(FILLS, "some")
    seven = SegmentTable(t.kind, t.ctrl, t.mat, t.sub_off, t.closed, t.mats, 100.0)                                          # the field comes last and has a default
    assert seven.fill_group is None and seven.canvas_height == 100.0


# ------------------------------------------------------------------ options
def test_options_parse_and_validate():
    from orip import svg as SV
    from test_svg_host import options_for
    d = SV.SvgOptions()
    assert (d.hatch_spacing_mm, d.hatch_inset_mm, d.hatch_direction, d.no_serpentine, d.hatch_fill) == (None, 27.0 / 40.0, "horizontal", False, "stated")
    assert SV.hatch_params(d) is None and SV.hatch_params(options_for(["--hatch-inset-mm", "1", "--hatch-direction", "cross"])) is None
    assert SV.hatch_params(options_for(["--hatch-spacing-mm", "0.5"])) == {"spacing": 20, "inset": 27, "flags": HD.HORIZONTAL | HD.SERPENTINE, "steps_per_mm": 40.0}
    p = SV.hatch_params(options_for(["--hatch-spacing-mm", "1.26", "--hatch-inset-mm", "0", "--hatch-direction", "cross", "--no-serpentine", "--steps-per-mm", "10"]))
    assert p == {"spacing": 13, "inset": 0, "flags": HD.HORIZONTAL | HD.VERTICAL, "steps_per_mm": 10.0}
    assert SV.hatch_params(options_for(["--hatch-spacing-mm", "1", "--hatch-direction", "vertical"]))["flags"] == HD.VERTICAL | HD.SERPENTINE
    assert SV.hatch_params(options_for(["--hatch-spacing-mm", "1", "--steps-per-mm", "5000"]))["spacing"] == 5000
    for bad in (["--hatch-spacing-mm", "0.01"], ["--hatch-spacing-mm", "0"], ["--hatch-spacing-mm", "-1"], ["--hatch-spacing-mm", "1", "--steps-per-mm", "5000.5"],
                ["--hatch-spacing-mm", "1", "--hatch-inset-mm", "-0.1"], ["--hatch-spacing-mm", "nan"]):
        with pytest.raises(ValueError):
            SV.hatch_params(options_for(bad))
    for bad in (["--hatch-direction", "diagonal"], ["--hatch-fill", "some"]):
        with pytest.raises(SystemExit):
            options_for(bad)
    g = SV.options_from_args(SV.build_gcode_argparser().parse_args(["x.svg", "--hatch-spacing-mm", "2", "--hatch-fill", "all"]))
    assert (g.hatch_spacing_mm, g.hatch_fill) == (2.0, "all")
    from orip import lib
    assert (lib.HATCH_SERPENTINE, lib.HATCH_HORIZONTAL, lib.HATCH_VERTICAL) == (HD.SERPENTINE, HD.HORIZONTAL, HD.VERTICAL)


# ------------------------------------------------------------------ the whole tool on the doubles
@pytest.mark.parametrize("i", [0, 3, 6, 9, 24, 28])
def test_tool_without_the_options_is_unchanged(i):
    from orip import svg as SV
    from test_svg_host import G, ARGS, RUNS, svg_text, options_for
    name, key = RUNS[i]

    def never(*a):
        raise AssertionError("hatching is off")
    data, info = SV.build_stream_from_svg(svg_text(name), options_for(ARGS[key]), want_paths=True, **dict(SD.svg_doubles(), hatch_fn=never))
    assert data == bytes(G[f"run_{i}_bin"]) and "hatch" not in info
    off, pts = info["fitted_paths"]
    assert SV.gcode_text(off, pts).encode() == bytes(G[f"run_{i}_gcode"])
    data, info = SV.build_stream_from_svg(svg_text(name), options_for(ARGS[key] + ["--hatch-inset-mm", "2", "--hatch-direction", "cross", "--hatch-fill", "all", "--no-serpentine"]),
                                          **dict(SD.svg_doubles(), hatch_fn=never))
    assert data == bytes(G[f"run_{i}_bin"])                                                   # the other options alone switch nothing on


def svg_of(polys, fill='fill="black"'):
    """the integer polygons (min x = min y = 0) as ONE path element whose fitted coordinates are k / 40 mm under --scale 0.025 --margin-mm 0"""
    h = int(max(p[:, 1].max() for p in polys))
    d = "".join("M" + "L".join(f"{x} {h - y}" for x, y in p.tolist()) + "Z" for p in polys)
    return f'<svg {NS} width="{int(max(p[:, 0].max() for p in polys))}" height="{h}"><path {fill} d="{d}"/></svg>'


TOOL = ["--scale", "0.025", "--margin-mm", "0", "--no-reorder"]


def run_tool(text, args, **kw):
    from orip import svg as SV
    from test_svg_host import options_for
    seen = {}
    base = SD.svg_doubles()

    def steps(paths, m):
        seen["steps"] = base["steps_fn"](paths, m); seen["map"] = m
        return seen["steps"]
    data, info = SV.build_stream_from_svg(text, options_for(TOOL + args), want_paths=True, **dict(base, hatch_fn=HD.hatch_numpy, steps_fn=steps, **kw))
    return data, info, seen


@pytest.mark.parametrize("name,invert", [("hole", 0), ("hole", 1), ("nested_overlapping", 0), ("islands_empty_lines", 1), ("inset_swallows", 0), ("comb_block", 0)])
def test_tool_with_hatching_gives_the_reference_integers(name, invert):
    from orip import svg as SV, gcode as GC
    polys, spacing, inset, serp, want = case(name)
    assert min(p[:, 0].min() for p in polys) == 0 == min(p[:, 1].min() for p in polys)
    args = ["--hatch-spacing-mm", repr(spacing / 40.0), "--hatch-inset-mm", repr(inset / 40.0), "--invert-y", str(invert)] + ([] if serp else ["--no-serpentine"])
    data, info, seen = run_tool(svg_of(polys), args)
    n_out = len(polys)
    assert info["hatch"]["segments"] == len(want) and info["hatch"]["groups"] == 1 and info["subpaths"] == n_out
    off, pts = seen["steps"]
    if invert:
        want = want.copy(); want[:, [1, 3]] = 11880 - 1 - want[:, [1, 3]]
    assert len(off) - 1 == n_out + len(want) and np.array_equal(np.diff(off)[n_out:], np.full(len(want), 2))
    assert np.array_equal(pts[off[n_out]:].reshape(-1, 4), want)                              # the stepped hatch paths ARE the reference's calls
    moff, mpts = info["fitted_paths"]
    text = SV.gcode_text(moff, mpts)
    goff, gpts, _ = GC.parse_gcode(text)                                                      # the written file says the same
    again = GD.to_steps_numpy(goff, gpts, seen["map"])
    assert np.array_equal(again[0], off) and np.array_equal(again[1], pts)
    plain, pinfo, pseen = run_tool(svg_of(polys), ["--invert-y", str(invert)])                # the outlines are what they are without hatching
    assert "hatch" not in pinfo and np.array_equal(pseen["steps"][1], pts[:off[n_out]]) and data != plain
    none, ninfo, _ = run_tool(svg_of(polys, ""), args)                                        # no fill written down: nothing to hatch
    assert ninfo["hatch"] == {"groups": 0, "lines": 0, "crossings": 0, "segments": 0} and none == plain
    allf, ainfo, _ = run_tool(svg_of(polys, ""), args + ["--hatch-fill", "all"])
    assert allf == data and ainfo["hatch"] == info["hatch"]


def test_tool_vertical_is_horizontal_of_the_transposed_drawing():
    polys = case("nested_overlapping")[0]
    args = ["--hatch-spacing-mm", "0.175", "--hatch-inset-mm", "0.075"]
    _, hi, hs = run_tool(svg_of([p[:, ::-1] for p in polys]), args)
    _, vi, vs = run_tool(svg_of(polys), args + ["--hatch-direction", "vertical"])
    n = len(polys)
    h, v = hs["steps"][1][hs["steps"][0][n]:].reshape(-1, 4), vs["steps"][1][vs["steps"][0][n]:].reshape(-1, 4)
    # the SVG's Y axis points down and the page's up: transposing the SVG mirrors the page drawing in both axes as well, so compare through the integers
    q = [p.copy() for p in polys]
    want_h = HD.hatch_segments(np.concatenate([[0], np.cumsum([len(p) for p in q])]), np.concatenate(q)[:, ::-1], [0] * n, 7, 3, HD.HORIZONTAL | HD.SERPENTINE)[0]
    assert len(v) and np.array_equal(v, want_h[:, [1, 0, 3, 2]]) and np.array_equal(h, want_h)
    _, ci, cs = run_tool(svg_of(polys), args + ["--hatch-direction", "cross"])
    c = cs["steps"][1][cs["steps"][0][n]:].reshape(-1, 4)
    hh = run_tool(svg_of(polys), args)[2]["steps"]
    assert np.array_equal(c, np.concatenate([hh[1][hh[0][n]:].reshape(-1, 4), v])) and ci["hatch"]["segments"] == len(c)


def test_tool_refuses_bad_hatch_options_before_any_device_step():
    from orip import svg as SV
    from test_svg_host import options_for

    def never(*a):
        raise AssertionError("refused before the device")
    for bad in (["--hatch-spacing-mm", "0.001"], ["--hatch-spacing-mm", "1", "--steps-per-mm", "6000"]):
        with pytest.raises(ValueError):
            SV.build_stream_from_svg(svg_of(case("hole")[0]), options_for(bad), flatten_fn=never, bbox_fn=never, fit_fn=never, hatch_fn=never, fetch_fn=never, steps_fn=never,
                                     order_fn=never, codes_fn=never, pack_fn=never)


def test_gcode_tool_writes_the_hatch_lines(tmp_path):
    from orip import svg as SV, gcode as GC
    polys, spacing, inset, serp, want = case("hole")
    src = tmp_path / "d.svg"; src.write_text(svg_of(polys))
    out = tmp_path / "d.gcode"
    R = dict(flatten_fn=SD.flatten_numpy, bbox_fn=SD.bbox_numpy, fit_fn=SD.fit_numpy, fetch_fn=SD.fetch_numpy, hatch_fn=HD.hatch_numpy)
    SV.main_gcode([str(src), "-o", str(out), "--scale", "0.025", "--margin-mm", "0", "--hatch-spacing-mm", "0.5", "--hatch-inset-mm", "0.075"], **R)
    off, pts, _ = GC.parse_gcode(out.read_text())
    assert np.array_equal(np.rint(pts[off[2]:] * 40.0).astype(np.int64).reshape(-1, 4), want)
    SV.main_gcode([str(src), "-o", str(tmp_path / "p.gcode"), "--scale", "0.025", "--margin-mm", "0"], **R)
    assert (tmp_path / "p.gcode").read_text() == SV.gcode_text(off[:3], pts[:off[2]])
