"""TEST INFRASTRUCTURE: the inputs of the --clip tests (tests/test_clip_host.py on the double, tests/test_gpu_clip.py on the device): the smallest shapes that
can break the rule or the kernel, on a sheet of 8 x 8 steps at one step per mm unless a case says otherwise; a random drawing with halves in the conversion
and in the cuts; and the drawings of the whole-tool tests.  A case is (off, pts_mm, map, rect)."""
import numpy as np

TOP = 1 << 30


def sheet_map(W=8, H=8, steps_per_mm=1.0, invert_y=0, **kw):
    return dict(dict(scale_x=1.0, scale_y=1.0, offset_x_mm=0.0, offset_y_mm=0.0, steps_per_mm=float(steps_per_mm), W=W, H=H, invert_y=invert_y), **kw)


def case(lists, m=None, rect=None):
    """[[(x, y) in mm, ...], ...] -> (off, pts_mm, map, rect); rect None: the sheet"""
    m = m or sheet_map()
    off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
    pts = np.asarray([q for p in lists for q in p], np.float64).reshape(-1, 2)
    return off, pts, m, tuple(rect) if rect is not None else (0, 0, m["W"] - 1, m["H"] - 1)


def both(*segs):
    """every segment as a path of its own, forwards and backwards"""
    return [list(s) for s in segs] + [list(s)[::-1] for s in segs]


# one segment inside each of the eight regions around [0, 7]^2, none touching it
REGIONS = [((-3, -3), (-1, -2)), ((2, -3), (5, -1)), ((9, -1), (12, -4)), ((-4, 2), (-1, 5)), ((8, 1), (11, 6)), ((-2, 9), (-1, 12)), ((1, 8), (6, 10)), ((9, 9), (8, 12))]
SEGMENTS = {
    "seg_inside": both(((1, 1), (6, 5))),
    "seg_outside_regions": both(*REGIONS),
    "seg_spans_two_regions": both(((-3, 1), (1, -3)), ((-5, 5), (4, 14))),                 # west to south and west to north, past the corners
    "seg_crosses_one_side": both(((3, 3), (10, 5)), ((3, 3), (4, -6)), ((-9, 0), (2, 7)), ((6, 6), (6, 20))),
    "seg_crosses_two_sides": both(((-2, 2), (10, 6)), ((-2, 3), (3, -2)), ((3, -5), (4, 12)), ((5, 9), (10, 4))),
    "seg_through_a_corner": both(((-2, -2), (3, 3)), ((9, -2), (-2, 9)), ((6, 6), (9, 9))),
    "seg_touches_a_corner": both(((5, 9), (9, 5)), ((-1, 1), (1, -1)), ((7, 7), (9, 12)), ((-3, 7), (0, 7), (0, 9))),      # a single point each: nothing is drawn
    "seg_along_the_border": both(((-2, 0), (10, 0)), ((-2, -1), (10, -1)), ((7, -3), (7, 3)), ((8, -3), (8, 3)), ((0, 0), (7, 0)), ((0, 7), (0, 0))),
    "seg_halves": both(((-1, 2), (1, 3)), ((-1, 3), (1, 2)), ((3, -1), (4, 1)), ((4, -1), (3, 1)), ((6, 2), (8, 3)), ((6, 3), (8, 2)), ((2, 6), (5, 8)), ((-3, 0), (3, 3)),
                       ((-1, 6), (1, 7)), ((6, 1), (8, 0))),
    "seg_cut_collapses": both(((-1, 1), (3, -2)), ((-1, 1), (2, -1)), ((8, 5), (5, 9)), ((6, 8), (8, 5))),      # a sliver of a corner: the first and the third round to one point
    "seg_degenerate": both(((3, 3), (3, 3)), ((9, 3), (9, 3)), ((7, 7), (7, 7)), ((0, -1), (0, -1))),
}


def zigzag(k, x_step=1.0, low=2.0, high=12.0):
    """k + 1 points that alternate between y = low (inside) and y = high (outside), x going right"""
    return [(j * x_step, high if j % 2 else low) for j in range(k + 1)]


def small_cases():
    """name -> (off, pts_mm, map, rect); every case also with invert_y (name + "_inv")"""
    c = {name: case(paths) for name, paths in SEGMENTS.items()}
    every = [p for paths in SEGMENTS.values() for p in paths]
    c.update({
        # (7, 4) lies on the border: the path leaves through it and comes back through it, and two strokes share it
        "path_out_and_back": case([[(2, 2), (7, 4), (10, 4), (7, 4), (2, 6)], [(2, 2), (7, 4), (10, 5), (7, 4), (2, 6)], [(3, 0), (3, -4), (3, 0), (3, 5)]]),
        "path_zigzag": case([[(1, 1), (6, 6)], zigzag(7) + [(7, 2)], [(6, 1), (1, 6)]]),                        # leaves and comes back four times: src = 0, 1 x 5, 2
        "path_repeats": case([[(2, 2), (2, 2), (5, 5), (5, 5), (9, 9), (9, 9), (9, 9), (5, 6), (5, 6)], [(-1, -1), (-1, -1)], [(4, 4), (4, 4), (4, 4)], [(7, 1), (7, 1), (9, 1), (9, 1), (7, 1)]]),
        "path_short_ones_between": case([[(1, 1), (9, 1)], [], [(3, 3)], [(2, 9), (2, 5), (9, 5)], [], [], [(12, 12)], [(5, 5), (6, 6)], []]),
        "path_only_short_ones": case([[], [(3, 3)], [(9, 9)]]),
        "path_only_empty_ones": case([[], []]),
        "path_phantom_join": case([[(-2, 2), (2, 2)], [(5, 5), (9, 5)], [(4, 9), (4, 6)], [(4, 1), (4, -3)]]),     # last point of one, first of the next: both inside, not a segment
        "path_600_points": case([zigzag(599, x_step=0.01, low=3.0, high=7.6)]),                                  # y = 7.6 rounds to 8, outside; x rounds to 0 .. 6
        "paths_300_of_two": case([[(-1 + 0.03 * j, (j * 5) % 11 - 1), (8 - 0.03 * j, (j * 3) % 12 - 2)] for j in range(300)]),
        "margin": case(every, rect=(2, 2, 5, 5)),
        "margin_zigzag": case([zigzag(7) + [(7, 2)]], rect=(1, 1, 6, 6)),
        "rect_of_one_point": case(every + [[(3, 3), (3, 3)], [(0, 0), (6, 6)], [(3, 0), (3, 7), (0, 3), (7, 3)]], rect=(3, 3, 3, 3)),
        "sheet_of_one_step": case(both(((-2, -2), (3, 3)), ((0, 0), (0, 0)), ((-1, 0), (1, 0)), ((-1, 1), (1, 0)), ((0, 0), (5, 1))) + [[(-1, 0), (0, 0), (0, 1), (0, 0), (0, 0)]], sheet_map(1, 1)),
        "half_steps": case(every, sheet_map(9, 9, 2.0, offset_x_mm=0.25)),                                       # k + 1/2 before the rounding, to even
        # coordinates at both ends of the range: a difference of 2^31, products of 2^62
        "overflow": case(both(((-TOP, -TOP + 1), (TOP, TOP)), ((-TOP, TOP), (TOP, -TOP)), ((-TOP, 3), (TOP, 4)), ((TOP, -TOP), (-TOP + 1, TOP))) + [[(-TOP, -TOP), (3, 3), (TOP, TOP - 1)]]),
        "overflow_large_sheet": case(both(((-TOP, -TOP + 1), (TOP, TOP)), ((-TOP, TOP), (TOP, -TOP)), ((-TOP, TOP - 5), (TOP, TOP - 6)), ((-TOP + 1, -TOP), (TOP, TOP - 1))),
                                     sheet_map(TOP, TOP), rect=(1, 0, TOP - 1, TOP - 2)),
    })
    for name in list(c):
        off, pts, m, rect = c[name]
        if name.startswith("overflow"):                                # mirrored in mm beforehand, so that (H - 1) - y stays inside the coordinate range
            pts = np.stack([pts[:, 0], float(m["H"] - 1) - pts[:, 1]], 1)
        c[name + "_inv"] = (off, pts, dict(m, invert_y=1), rect)
    c["nothing"] = case([])
    return c


def range_error_case():
    """one coordinate is 2^30 + 1 after the rounding"""
    return case([[(1, 1), (6, 6)], [(2, 2), (TOP + 1, 3)]])


def random_case(seed=5, n=2000):
    """2000 paths of 2 .. 6 points on a sheet of 9 x 9 steps at 2 steps per mm; every coordinate a multiple of 0.25 mm in [-12, 20], so halves occur in the
    conversion (round to even) and in the cuts (toward +infinity).  Half of the paths start near the sheet and every path wanders by up to 3 mm a point, so
    that whole, cut and outside segments all occur in number."""
    rng = np.random.default_rng(seed)
    lists = []
    for _ in range(n):
        k = int(rng.integers(2, 7))
        p = rng.integers(-8, 29, 2) if rng.random() < 0.5 else rng.integers(-48, 81, 2)           # quarters of a mm
        pts = [p]
        for _ in range(k - 1):
            p = np.clip(p + rng.integers(-12, 13, 2), -48, 80)
            pts.append(p)
        lists.append([(float(q[0]) * 0.25, float(q[1]) * 0.25) for q in pts])
    return case(lists, sheet_map(9, 9, 2.0))


# ------------------------------------------------------------------ the drawings of the whole-tool tests
def circle_gcode(cx=0.0, cy=60.0, r=40.0, k=90):
    """a circle of radius 40 mm around (0, 60): its left half is off an A4 sheet; and a square well inside that sheet"""
    out = ["G21", "G90", "M5"]
    pts = [(cx + r * np.cos(2 * np.pi * j / k), cy + r * np.sin(2 * np.pi * j / k)) for j in range(k + 1)]
    sq = [(100, 100), (150, 100), (150, 150), (100, 150), (100, 100)]
    for s in (pts, sq):
        out += ["G0 X%.4f Y%.4f" % s[0], "M3"] + ["G1 X%.4f Y%.4f" % q for q in s[1:]] + ["M5"]
    return "\n".join(out) + "\n"


# the same circle on a sheet of 400 x 300 steps at 4 steps per mm, which a preview shows one step to the pixel; the square is then off the sheet altogether
PREVIEW_GCODE_ARGS = dict(steps_per_mm=4.0, target_width_steps=400, target_height_steps=300)


def preview_gcode():
    return circle_gcode(0.0, 37.5, 25.0)


def inside_gcode():
    """a drawing that stays on the sheet: three pens, strokes that meet end to end"""
    out = ["G21", "G90", "M5"]
    for t, s in ((1, [(10, 10), (60, 10), (60, 60)]), (1, [(60, 60), (10, 60), (10, 10)]), (2, [(100, 20), (120, 40)]), (0, [(30, 200), (90, 250), (150, 200)]), (2, [(120, 40), (140, 20)])):
        out += ["T%d" % t, "G0 X%g Y%g" % s[0], "M3"] + ["G1 X%g Y%g" % q for q in s[1:]] + ["M5"]
    return "\n".join(out) + "\n"


# scaled by 3 on a page of 100 x 100 mm the drawing is wider and higher than the page (the fit puts its lower left corner on the page's); the filled circle
# hangs over the right edge
TOOL_SVG = b"""<svg xmlns="http://www.w3.org/2000/svg" width="100" height="100" viewBox="0 0 100 100">
 <circle cx="23" cy="15" r="12" fill="#00f" stroke="#00f"/>
 <path stroke="#f00" fill="none" d="M-10 5 L40 5 L40 30 L-10 30"/>
 <polyline stroke="#f00" fill="none" points="5,2 10,40 15,2 20,40 25,2"/>
 <line x1="2" y1="20" x2="30" y2="20" stroke="#0f0"/>
</svg>
"""
TOOL_SVG_ARGS = ["--page-width-mm", "100", "--page-height-mm", "100", "--margin-mm", "0", "--scale", "3", "--steps-per-mm", "10", "--clip"]
TOOL_SVG_INSIDE_ARGS = ["--page-width-mm", "100", "--page-height-mm", "100", "--steps-per-mm", "10"]          # the automatic fit: everything on the page
