"""TEST INFRASTRUCTURE: the stroke passes in combination.  Two drawings (one per vector front door) on which every pass has work whenever its option is on,
the options of each door as factors with levels of command-line words, the one predicate that says which combinations the front doors refuse, a seeded
greedy generator of covering arrays over the factors, and the two functions that put EVERY device step of a door on the CPU (the doubles of tests/*_double.py
composed, nothing else).  Plain data and numpy; tests/test_compose_host.py holds the drawings and the rows to what they are built for, on the CPU, and
tests/test_gpu_compose.py runs every row on the device against the all-double run.

Rows.  Strength 2 over all factors of a door, strength 3 over the stroke-rewriting subset (SVG: clip, dash, hatch-connect, occlude, dedup, merge, simplify;
G-code: clip, dash, dedup, merge, simplify), the all-on and the all-off row added by hand, at most 96 rows per door.  Counts and times as generated
(ROW_COUNTS below, which test_compose_host.py asserts; the times are those of the all-double run on the CPU this was written on, the bound is 2 s):

    SVG door     30 rows     slowest all-double row 0.60 s: --allow-reverse --ring-entry --improve-order --loop-start --clip --dashes --hatch-spacing-mm 8
                             --no-serpentine --hatch-connect --dedup --merge-paths --stipple-mm 12 --stipple-pattern square
    G-code door  30 rows     slowest all-double row 0.30 s: --improve-order --clip --clip-margin-mm 4 --dash-mm 6,3 --dedup

No row has more than 271 strokes and dots (SVG door) or 178 (G-code door); MAX_OPS below is the bound the host test holds them to.

Refused combinations (each raises ValueError from the front door and is in no row): --no-reorder with --improve-order or --ring-entry; --hatch-connect
without a hatch; --clip-margin-mm without --clip; --dash-offset-mm without --dash-mm; --hatch-connect-mm without --hatch-connect; --stipple-inset-mm or
--stipple-pattern without --stipple-mm; --improve-rounds without --improve-order; a --pen-order that names a pen twice or outside 0..7.  No combination
of the factors below turned out to be refused beyond these, no row disagreed between the device and the doubles, and nothing had to be fixed.

One consequence the rows brought out, which is the stream compiler's rule and not a fault: a segment drawn backwards (--allow-reverse) does not ink the
same lattice steps as the segment drawn forwards.  The walk takes round-half-down of k d / D from the segment's FIRST point, so where the exact line
passes midway between two lattice points the two directions choose different ones ((0, 0) -> (4, 2) passes (1, 0) and (3, 1), (4, 2) -> (0, 0) passes
(3, 2) and (1, 1)).  test_compose_host.py therefore compares the inked steps exactly wherever neither run may reverse a stroke, and within one lattice
step, pen by pen, with equal pen-down step counts, where one may."""
import itertools

import numpy as np

# ------------------------------------------------------------------ the drawings
# The SVG drawing, in page mm (--scale 1 --margin-mm 0: the box of the drawing goes to the sheet's corner; the anchor stroke from (0, 297) keeps SVG x and
# 297 - y the page coordinates).  The sheet is 210 x 297 mm.  Elements in paint order:
#   anchor     a short black stroke from the drawing's corner: the box starts at (0, 0), and a fourth stroke colour, nearest to no pen in particular
#   dashed     a long blue stroke with stroke-dasharray 6 3 (21 dashes) that passes under C: dashes cut and hidden by a shape
#   under      a short red stroke wholly under C: a hidden segment whatever else is on
#   reach      a blue stroke that ends under the triangle, 1 mm inside the sheet's edge: under --occlude --clip it is cut by a ring that is not clamped
#   A, B       two filled rectangles, both outlined in blue, that share the border x = 80: dedup (unless C hides it: the green pair below stays)
#   C          a filled green rectangle over A's and B's corners, the dashed stroke and `under`: occlusion cuts, hidden hatch lines and hidden dots
#   U          a concave filled shape whose legs stand 8 mm apart: hatch lines across the slit are within reach of each other and may not link
#   grey       a shape with a fill and no stroke colour: it takes --color-index, a pen of its own
#   triangle   a filled red shape half off the sheet (its apex at x = 260): clip cuts, and rings converted without the clamp
#   ring, tail red <line>s that meet end to end: four close into a ring (merge cycles), two stay an open chain (merge joins); nothing covers them
#   pair       two green collinear strokes that overlap from x = 50 to 80: dedup whatever --occlude hides
#   bezier     a green cubic flattened to half a step: more points than --simplify-mm 0.1 needs
#   steps      a green polyline with a vertex on the straight line between its neighbours: --simplify-mm 0 drops it
#   circles    three unfilled red circles that nothing covers, their first vertices (the rightmost) away from where the pen arrives: ring entry and seams
SVG_TEXT = b"""<svg xmlns="http://www.w3.org/2000/svg" width="260" height="297" viewBox="0 0 260 297">
 <path d="M0 297 L8 290" stroke="#000" fill="none"/>
 <path d="M5 100 H200" stroke="#00f" stroke-dasharray="6 3" fill="none"/>
 <line x1="70" y1="80" x2="100" y2="90" stroke="#f00"/>
 <path d="M150 175 H209" stroke="#00f" fill="none"/>
 <rect x="20" y="20" width="60" height="50" fill="#88f" stroke="#00f"/>
 <rect x="80" y="20" width="50" height="50" fill="#f88" stroke="#00f"/>
 <rect x="50" y="45" width="60" height="70" fill="#8f8" stroke="#0f0"/>
 <path d="M20 130 H120 V220 H74 V160 H66 V220 H20 Z" fill="#88f" stroke="#00f"/>
 <rect x="136" y="62" width="28" height="28" fill="#ccc"/>
 <path d="M180 150 L260 172 L180 200 Z" fill="#f88" stroke="#f00"/>
 <g stroke="#f00"><line x1="140" y1="232" x2="170" y2="232"/><line x1="170" y1="232" x2="170" y2="258"/><line x1="170" y1="258" x2="140" y2="258"/>
  <line x1="140" y1="258" x2="140" y2="232"/><line x1="150" y1="270" x2="180" y2="270"/><line x1="180" y1="270" x2="195" y2="285"/></g>
 <line x1="10" y1="240" x2="80" y2="240" stroke="#0f0"/><line x1="50" y1="240" x2="120" y2="240" stroke="#0f0"/>
 <path d="M10 285 C40 245 80 300 125 262" stroke="#0f0" fill="none"/>
 <polyline points="10,228 40,228 70,228 70,235" stroke="#0f0" fill="none"/>
 <circle cx="160" cy="30" r="14" fill="none" stroke="#f00"/><circle cx="190" cy="118" r="12" fill="none" stroke="#f00"/>
 <circle cx="195" cy="250" r="10" fill="none" stroke="#f00"/>
</svg>
"""
SVG_HEIGHT_MM, SVG_STEPS_PER_MM = 297.0, 10
# the filled shapes of SVG_TEXT in paint order, as polygons in SVG user units: what a dot may not lie in when the shape is painted after the dot's own
SVG_FILLED = [("A", [(20, 20), (80, 20), (80, 70), (20, 70)]), ("B", [(80, 20), (130, 20), (130, 70), (80, 70)]), ("C", [(50, 45), (110, 45), (110, 115), (50, 115)]),
              ("U", [(20, 130), (120, 130), (120, 220), (74, 220), (74, 160), (66, 160), (66, 220), (20, 220)]), ("grey", [(136, 62), (164, 62), (164, 90), (136, 90)]),
              ("triangle", [(180, 150), (260, 172), (180, 200)])]
SVG_FILL_PEN = [0, 1, 2, 0, 0, 1]       # the pen of each shape's dots under --pen-colors #00f,#f00,#0f0 (the grey is as far from all three: the lowest)
SVG_BASE = ["--scale", "1", "--margin-mm", "0", "--steps-per-mm", str(SVG_STEPS_PER_MM)]


def _gcode_text() -> str:
    """The G-code drawing, in mm on an A4 sheet (210 x 297).  Paths in file order:
      before any T   a short stroke that takes --color-index under --tool-pens: a fourth pen
      T0  square, hexagon   closed loops listed from the vertex farthest from the origin: ring entry and seams
          pair              two collinear strokes that overlap from x = 80 to 120: dedup, dashed or not
          long              400 mm in three segments: some forty dashes of --dash-mm 6,3
      T1  ring, tail        pieces of 30 mm that meet end to end (a dash of 6,3 ends at 30 mm and one starts at 0, with or without the offset of 2): four
                            close into a ring, two stay an open chain
          noisy             a polyline of 2 mm chords whose vertices lie on the line or one step off it: --simplify-mm 0.1 and 0 both drop some
      T2  triangle          a closed loop
          out, left         strokes that leave the sheet at x = 210 and at x = 0: clip cuts, and clamped points otherwise
          two tiny squares  closed loops of 3.6 mm, shorter than what is left of the first dash under either --dash-mm level (6 mm, or 4 behind the offset): they
                            stay closed when everything else is dashed, so ring entry and seams have work in every row"""
    out = ["G21 G90"]

    def path(pts):
        out.append("G0 X%g Y%g" % pts[0]); out.append("M3")
        out.extend("G1 X%g Y%g" % p for p in pts[1:]); out.append("M5")
    path([(5, 5), (15, 8)])
    out.append("T0")
    path([(70, 70), (30, 70), (30, 30), (70, 30), (70, 70)])
    hexagon = [(150 + 25 * c, 60 + 25 * s) for c, s in ((1, 0), (0.5, 0.866), (-0.5, 0.866), (-1, 0), (-0.5, -0.866), (0.5, -0.866))]
    path(hexagon[1:] + hexagon[:2])
    path([(20, 100), (120, 100)]); path([(80, 100), (180, 100)])
    path([(10, 120), (200, 120), (200, 140), (10, 140)])
    out.append("T1")
    for a, b in (((30, 160), (60, 160)), ((60, 160), (60, 190)), ((60, 190), (30, 190)), ((30, 190), (30, 160)), ((100, 160), (130, 160)), ((130, 160), (145, 190))):
        path([a, b])
    noise = (0, 0, 0, 0.1, 0, 0, 0, -0.1)
    path([(10 + 2 * k, 220 + noise[k % 8]) for k in range(71)])
    out.append("T2")
    path([(160, 280), (130, 240), (190, 240), (160, 280)])
    path([(190, 200), (230, 210), (190, 220)]); path([(-10, 260), (40, 260), (40, 270)])
    path([(100.9, 200.9), (100, 200.9), (100, 200), (100.9, 200), (100.9, 200.9)]); path([(120, 250), (120.9, 250), (120.9, 250.9), (120, 250.9), (120, 250)])
    return "\n".join(out) + "\n"


GCODE_TEXT = _gcode_text()
GCODE_BASE = ["--steps-per-mm", "10"]

# ------------------------------------------------------------------ factors: name -> levels, each level a list of command-line words; level 0 is "off"
SVG_FACTORS = {
    "pens": [[], ["--pen-colors", "#00f,#f00,#0f0"], ["--pen-colors", "#00f,#f00,#0f0", "--pen-order", "2,0,3,1"]],
    "reverse": [[], ["--allow-reverse"]],
    "order": [[], ["--no-reorder"], ["--ring-entry"]],
    "improve": [[], ["--improve-order"]],
    "loop": [[], ["--loop-start"]],
    "clip": [[], ["--clip"], ["--clip", "--clip-margin-mm", "4"]],
    "dash": [[], ["--dashes"]],
    "hatch": [[], ["--hatch-spacing-mm", "8"], ["--hatch-spacing-mm", "8", "--hatch-direction", "cross"], ["--hatch-spacing-mm", "8", "--hatch-angle-deg", "30"],
              ["--hatch-spacing-mm", "8", "--hatch-angle-deg", "30", "--hatch-direction", "cross"], ["--hatch-spacing-mm", "8", "--no-serpentine"]],
    "connect": [[], ["--hatch-connect"]],
    "occlude": [[], ["--occlude"]],
    "dedup": [[], ["--dedup"]],
    "merge": [[], ["--merge-paths"]],
    "simplify": [[], ["--simplify-mm", "0"], ["--simplify-mm", "0.1"]],
    "stipple": [[], ["--stipple-mm", "12"], ["--stipple-mm", "12", "--stipple-pattern", "square"]],
    "invert_y": [[], ["--invert-y", "1"]],
}
GCODE_FACTORS = {
    "pens": [[], ["--tool-pens"], ["--tool-pens", "--pen-order", "2,0,3,1"]],
    "reverse": [[], ["--allow-reverse"]],
    "order": [[], ["--no-reorder"], ["--ring-entry"]],
    "improve": [[], ["--improve-order"]],
    "loop": [[], ["--loop-start"]],
    "clip": [[], ["--clip"], ["--clip", "--clip-margin-mm", "4"]],
    "dash": [[], ["--dash-mm", "6,3"], ["--dash-mm", "6,3", "--dash-offset-mm", "2"]],
    "dedup": [[], ["--dedup"]],
    "merge": [[], ["--merge-paths"]],
    "simplify": [[], ["--simplify-mm", "0"], ["--simplify-mm", "0.1"]],
    "invert_y": [[], ["--invert-y", "1"]],
}
FACTORS = {"svg": SVG_FACTORS, "gcode": GCODE_FACTORS}
BASE = {"svg": SVG_BASE, "gcode": GCODE_BASE}
REWRITING = {"svg": ("clip", "dash", "connect", "occlude", "dedup", "merge", "simplify"), "gcode": ("clip", "dash", "dedup", "merge", "simplify")}
REORDER_ONLY = ("reverse", "order", "improve", "loop")           # and the --pen-order of the pens factor: they change the sequence, not what is drawn
NO_REORDER, RING_ENTRY = 1, 2                                   # levels of "order"
ALL_ON = {"svg": dict(pens=2, reverse=1, order=2, improve=1, loop=1, clip=2, dash=1, hatch=4, connect=1, occlude=1, dedup=1, merge=1, simplify=2, stipple=1, invert_y=1),
          "gcode": dict(pens=2, reverse=1, order=2, improve=1, loop=1, clip=2, dash=2, dedup=1, merge=1, simplify=2, invert_y=1)}
MAX_ROWS = 96
ROW_COUNTS = {"svg": 30, "gcode": 30}                            # what generate_rows gives today; a change of the factors or of the generator changes them knowingly
MAX_OPS = 300                                                   # strokes plus dots of any row: the improve double is brute force


def allowed(door: str, levels: dict) -> bool:
    """THE predicate: False iff the front door refuses the levels given (a partial assignment is judged on what it states).  Read off orip.gcode.stroke_options
    (--no-reorder with --improve-order or with --ring-entry; the level --ring-entry excludes --no-reorder by being another level of the same factor) and
    orip.svg.hatch_connect_reach (--hatch-connect needs a hatch).  A margin, a dash offset, a pen order, a stipple pattern and a hatch direction stand only in
    levels that also hold the option they belong to, so the refusals of a lone one (REFUSED below) cannot occur in a row."""
    if levels.get("order") == NO_REORDER and levels.get("improve"):
        return False
    if door == "svg" and levels.get("connect") and levels.get("hatch") == 0:
        return False
    return True


# word lists every one of which the door refuses with a ValueError, the three of the predicate first
REFUSED = {
    "svg": [["--no-reorder", "--improve-order"], ["--no-reorder", "--ring-entry"], ["--hatch-connect"], ["--clip-margin-mm", "4"], ["--hatch-connect-mm", "5", "--hatch-spacing-mm", "8"],
            ["--stipple-pattern", "square"], ["--stipple-inset-mm", "1"], ["--improve-rounds", "3"], ["--pen-colors", "#00f", "--pen-order", "1,1"]],
    "gcode": [["--no-reorder", "--improve-order"], ["--no-reorder", "--ring-entry"], ["--clip-margin-mm", "4"], ["--dash-offset-mm", "2"], ["--improve-rounds", "3"],
              ["--tool-pens", "--pen-order", "8"]],
}


def words(door: str, row: dict) -> list:
    """the command-line words of a row, the door's base first"""
    return BASE[door] + [w for name, levels in FACTORS[door].items() for w in levels[row[name]]]


def options(door: str, row_or_words):
    """the parsed options of a row (or of extra words behind the door's base)"""
    w = words(door, row_or_words) if isinstance(row_or_words, dict) else BASE[door] + list(row_or_words)
    if door == "svg":
        from orip import svg as SV
        return SV.options_from_args(SV.build_stream_argparser().parse_args(["in.svg", "--no-preview"] + w))
    from orip import gcode as GC
    return GC.options_from_args(GC.build_argparser().parse_args(["in.gcode"] + w))


def tuples_to_cover(door: str):
    """every allowed pair of levels over all factors and every allowed triple over the rewriting subset, as frozensets of (factor, level)"""
    F = FACTORS[door]
    need = set()
    for names in list(itertools.combinations(F, 2)) + list(itertools.combinations(REWRITING[door], 3)):
        for lv in itertools.product(*(range(len(F[n])) for n in names)):
            t = dict(zip(names, lv))
            if allowed(door, t) and _extends(door, t) is not None:
                need.add(frozenset(t.items()))
    return need


def _extends(door: str, partial: dict, rng=None):
    """a full allowed row that holds `partial`, the other factors drawn by rng (None: their lowest allowed levels); None when there is none"""
    F = FACTORS[door]
    row = dict(partial)
    for name in F:
        if name in row:
            continue
        lv = list(range(len(F[name])))
        if rng is not None:
            lv = [lv[i] for i in rng.permutation(len(lv))]
        for v in lv:
            if allowed(door, dict(row, **{name: v})) and (name != "hatch" or not row.get("connect") or v):
                row[name] = v
                break
        else:
            return None
    return row if allowed(door, row) else None


def covered_by(door: str, row: dict):
    F = FACTORS[door]
    out = {frozenset(((a, row[a]), (b, row[b]))) for a, b in itertools.combinations(F, 2)}
    return out | {frozenset((n, row[n]) for n in names) for names in itertools.combinations(REWRITING[door], 3)}


def generate_rows(door: str, seed: int = 20240) -> list:
    """the row list of a door: the all-off and the all-on row, then greedily, from a seeded generator, the row that covers most of what is still uncovered
    among 48 candidates, each grown from an uncovered tuple.  Deterministic; every row satisfies allowed()."""
    F = FACTORS[door]
    rng = np.random.default_rng(seed)
    rows = [{n: 0 for n in F}, dict(ALL_ON[door])]
    need = tuples_to_cover(door)
    for r in rows:
        need -= covered_by(door, r)
    while need:
        pending = sorted(need, key=lambda t: sorted(t))
        best, gain = None, -1
        for _ in range(48):
            cand = _extends(door, dict(pending[int(rng.integers(len(pending)))]), rng)
            if cand is None:
                continue
            g = len(covered_by(door, cand) & need)
            if g > gain:
                best, gain = cand, g
        rows.append({n: int(best[n]) for n in F})
        need -= covered_by(door, best)
    return rows


_ROWS = {}


def rows(door: str) -> list:
    if door not in _ROWS:
        _ROWS[door] = generate_rows(door)
    return [dict(r) for r in _ROWS[door]]


def sibling(door: str, row: dict, **change) -> dict:
    """the row with the given factors at other levels"""
    return dict(row, **change)


def reorder_off(row: dict) -> dict:
    """the row with the options that only reorder off: greedy order, nothing reversed, no improvement, no seams, --pen-order ascending"""
    return dict(row, reverse=0, order=0, improve=0, loop=0, pens=min(row["pens"], 1))


# ------------------------------------------------------------------ every device step on the CPU
def _improve(ends, group, n_groups, order, rev, reverse, max_rounds):
    import improve_double as ID
    return ID.improve(ends, group, n_groups, order, rev, reverse, (0, 0), max_rounds)


def _seams(off, pts, order, rev):
    import seam_double as SM
    return SM.seams(off, pts, order, rev, (0, 0))


def _stroke_doubles():
    import dash_double as DH
    import dedup_double as DD
    import ring_entry_double as RD
    import simplify_double as SP
    return dict(dedup_fn=DD.dedup_numpy, simplify_fn=SP.simplify_numpy, dash_fn=DH.dash_numpy, seam_fn=_seams, ring_entry_fn=RD.order_rings_fn, improve_fn=_improve)


def svg_doubles_all(angle: bool) -> dict:
    """the keyword arguments that put every device step of orip.svg.build_stream_from_svg on the CPU, whatever options are on; angle: the hatch is
    --hatch-angle-deg's (orip_svg_hatch_angle stands in orip_svg_hatch's place on the device, and hatch_angle_double in hatch_double's here).  A new set per
    run: the doubles of the conversion, the hatch and the ring passes keep what the step behind them asks for."""
    import clip_double as CD
    import hatch_link_cases as LC
    import occlude_cases as OC
    import stipple_cases as TC
    d = dict(CD.svg_doubles(), occlude_fn=OC.OccludeDouble(), stipple_fn=TC.StippleDouble(), hatch_link_fn=LC.HatchLinkDouble(), **_stroke_doubles())
    if angle:
        import hatch_angle_double as HA
        H = HA.HatchAngleWithGroups()
        d.update(hatch_fn=H.hatch, hatch_groups_fn=H.hatch_groups)
    return d


def gcode_doubles_all() -> dict:
    """the same for orip.gcode.build_stream_from_gcode"""
    import clip_double as CD
    return dict(CD.gcode_doubles(), **_stroke_doubles())


def run_doubles(door: str, row_or_words, want_paths: bool = False):
    """(bytes, info) of a row through the doubles alone"""
    o = options(door, row_or_words)
    if door == "svg":
        from orip import svg as SV
        return SV.build_stream_from_svg(SVG_TEXT, o, want_paths=want_paths, **svg_doubles_all(o.hatch_angle_deg is not None and o.hatch_spacing_mm is not None))
    from orip import gcode as GC
    return GC.build_stream_from_gcode(GCODE_TEXT, o, **gcode_doubles_all())


def run_device(door: str, row_or_words, dev, want_paths: bool = False):
    """(bytes, info) of a row on the device: no step is given"""
    o = options(door, row_or_words)
    if door == "svg":
        from orip import svg as SV
        return SV.build_stream_from_svg(SVG_TEXT, o, dev, want_paths=want_paths)
    from orip import gcode as GC
    return GC.build_stream_from_gcode(GCODE_TEXT, o, dev)


# ------------------------------------------------------------------ comparing two runs
PASS_ORDER = ("segments", "subpaths", "canvas_height", "bbox", "scale", "tol_raw", "hatch", "hatch_u", "pen_colors", "path_pens", "fitted_paths", "paths_mm", "pen_down_moves",
              "target", "clip", "pens", "dash", "hatch_link", "occlude", "dedup", "merge", "simplify", "stipple", "taps", "ring_entry", "improve", "reversed", "seam", "paths",
              "moves", "pieces", "steps", "bytes")


def same_value(a, b) -> bool:
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys() and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and any(isinstance(v, np.ndarray) for v in list(a) + list(b)):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return type(a) is type(b) and a == b if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) else a == b


def first_difference(got: dict, want: dict):
    """the first key of info, in pass order, that one run has and the other has not or that differs: (key, got, want), or None"""
    keys = [k for k in PASS_ORDER if k in got or k in want] + sorted(k for k in set(got) | set(want) if k not in PASS_ORDER)
    for k in keys:
        if k not in got or k not in want or not same_value(got[k], want[k]):
            return k, got.get(k, "<absent>"), want.get(k, "<absent>")
    return None


def mismatch(door: str, row, got, info, want, winfo) -> str:
    """"" when the two runs agree in bytes and in every key of info, else the report of a failure: the row's words and the first key that differs"""
    diff = first_difference(info, winfo)
    if got == want and diff is None:
        return ""
    w = words(door, row) if isinstance(row, dict) else list(row)
    at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    return (f"{door}: {' '.join(w)}\n  bytes: {len(got)} against {len(want)}, first difference at {at}\n  first info key that differs, in pass order: " +
            (f"{diff[0]}: device {diff[1]!r}, doubles {diff[2]!r}" if diff else "none"))
