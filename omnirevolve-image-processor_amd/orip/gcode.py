"""G-code -> plotter stream: the second front door of the reference (svg_to_stream/gcode2stream.py), same wire format as stage 13 (orip/stream.py).

Four steps.  The text is parsed on the host into pen-down paths in mm (cheap: a pass over the lines).  The paths become step polylines on the device
(orip_gcode_to_steps), are put into nearest-neighbour order there (orip_gcode_order: the reference's O(n^2) Python scan is its dominant cost) and the
host plans the stream: every move of the plot (a travel to each path, then its segments), the speed pieces of every move with the plans of
orip/stream.py, and the byte position of every piece -- flat numpy over ALL paths, no Python call per segment.  The direction codes
(orip_stream_codes) stay on the device; orip_stream_pack writes the bytes there and only the finished stream comes back.

Everything that decides a byte follows the reference in meaning: comment and word rules of the parser, unit and mode switches inside a line, pen
state before motion, float64 arithmetic of the conversion, round half to even, the (L1 distance, index) order, the command sequence of the emitter,
the dividers after --speed-scale.  The device steps are injectable so that this host logic can be tested without a GPU; the product has no CPU path.

Pens (ours on this front door; the reference's gcode2stream.py draws everything with --color-index).  With a pen per path (--tool-pens: the T words of
the text; svg2stream --pen-colors: the stroke colours) the paths are drawn pen after pen, in --pen-order, each pen's paths in nearest-neighbour order from
where the pen before it stopped, with one colour byte per pen: draw_color_group of the reference's demo sheet (stream_generators/plotter_demo/
omnirevolve_plotter_demo.py :317-333) called for one pen after the other.  --allow-reverse lets that order draw a stroke backwards when its far end is
nearer (the demo's order_paths_nearest :197-216); both run on the device (orip_gcode_order_pens).  Without these options nothing changes.

--merge-paths (ours as well): step polylines of one pen that meet end to end -- every <line> of a CAD export, a path cut at every M, G-code that lifts the
pen at every vertex -- become one stroke before any order (orip_gcode_merge; include/orip.h states the rule), so the pen stays down across the joint and the
joint gets the corner slow-down of a vertex instead of a stop and a start.  Coincidence is on the step grid, without a tolerance; where three or more ends
meet nothing is joined.  Without the option no device call is added and every byte is what it was.

--improve-order (ours as well): the greedy order looks one step ahead; this option then lowers the pen-up steps of the plot, max(|dx|, |dy|) per travel as the
stream compiler counts them, by steepest descent over two kinds of move inside a pen's group: a run of strokes drawn in reverse order and direction (2-opt,
only with --allow-reverse) and a block of one to three strokes put elsewhere (or-opt).  One move per round, the best of all, ties by a fixed order; at most
--improve-rounds rounds per group (default 2 m + 64 for m strokes); groups of more than 65 536 strokes are left as they are (orip_gcode_improve;
include/orip.h states the rule).  It runs after the order and, with --merge-paths, on the merged strokes.  Without the option no device call is added.

--clip (ours as well): the reference clamps every point to the sheet (mm_to_steps / clamp_xy), so whatever leaves the sheet is drawn along the edge of the
paper, and a segment with one end outside changes its slope.  With --clip the strokes are cut where they cross the rectangle [m, W - 1 - m] x [m, H - 1 - m]
in steps, m = --clip-margin-mm in steps (default 0: the sheet); what lies outside is not drawn and the pen is lifted there (orip_gcode_to_steps_clip, which
takes the place of orip_gcode_to_steps; include/orip.h states the rule, exact in integers on the step grid).  A path that leaves and comes back becomes
several strokes of the same input path, so pens, merge, order and improve work on the cut strokes unchanged.  Without the option no device call is added
and every byte is what it was.

--simplify-mm (ours as well): every vertex of the input goes into the stream, as a move of its own, a speed byte and a candidate corner, and a segment of at
most --short-len-steps is drawn at --short-div; a curve flattened into chords the pen cannot resolve is drawn slower and in more bytes than it need be.  With
--simplify-mm T the vertices that lie within T of the stroke are dropped: Ramer-Douglas-Peucker per stroke on the step grid, exact in integers, the tolerance
in quarter steps, tol4 = round(4 T steps_per_mm) (orip_gcode_simplify; include/orip.h states the rule).  0 is allowed: it removes exactly the vertices on
the segment between their kept neighbours.  It runs after the merge, so that the joints inside a merged chain can go, and before the order; strokes, their
ends, pens and sources do not change.  Without the option no device call is added and every byte is what it was.

--dedup (ours as well): a map exported as one closed polygon per region, a table made of rectangles, a wall drawn over the walls it joins, a tracer that
walks a thin feature out and back -- all hold the same line twice, and the second pass is a darker, wider line, a tear with a wet pen, and pen-down time.
With --dedup collinear segments of one pen that lie over each other on the step grid are drawn once: the first drawn copy stays, of a later one only the
stretches nothing earlier covers, cut at end points of the input (orip_gcode_dedup; include/orip.h states the rule, exact in integers, no tolerance).  It
runs after the pens have been worked out and before the merge, which joins the pieces it leaves, and before the simplification, which would move two copies
of a shared border apart.  A stroke can be cut into several and can vanish; pens and sources follow.  Allowed with --no-reorder: strokes keep file order.
Without the option no device call is added and every byte is what it was.

--dash-mm (ours as well; svg2stream --dashes honours the drawing's own stroke-dasharray through the same pass): G-code has no notion of a dash, so a
perforation, a fold line or a stitch line is asked for here.  Every stroke is cut into the dashes of the pattern, measured along the stroke in 1/256 step
from its first point (--dash-offset-mm: from that far into the pattern): orip_gcode_dash; include/orip.h states the rule, exact in integers on the step
grid.  It runs after the pens have been worked out and before the occlusion and the dedup; every stroke the conversion leaves starts the pattern anew, so
under --clip the phase restarts at the sheet's edge, and the merge, which runs later, does not carry it on.  A dash keeps its stroke's pen and source; a
dash that rounds onto one grid point is dropped.  Without the option no device call is added and every byte is what it was.

--hatch-connect (svg2stream.py's; ours as well): every hatch line is a stroke of its own, so a hatched sheet lifts the pen once per line.  The pass joins
consecutive hatch lines of one shape and one hatch family into zigzags, by straight links of at most --hatch-connect-mm that lie wholly inside the shape
(orip_svg_hatch_link; include/orip.h states the rule, exact in integers on the step grid).  It runs after the pens and the dashes and before the occlusion,
the dedup, the merge and the simplification: it sees the hatch lines whole, and a shape on top cuts a zigzag as it cuts any ink.  Pen, level, dash pattern
and source follow a zigzag through its first line.  Without the option no device call is added and every byte is what it was.

--loop-start (ours as well): a circle, a rectangle, a closed path and a ring --merge-paths has rebuilt are entered and left at the vertex their file happened
to list first, and the orders and --improve-order see such a stroke as that one point.  With --loop-start every closed stroke (four points or more, the
first equal to the last) starts and ends at the ring vertex that makes the pen-up steps of the whole plot least, all closed strokes chosen together and
exactly, ties to the lowest vertex in drawing order (orip_gcode_seam; include/orip.h states the rule).  It runs after the order and after --improve-order,
immediately before the paths are gathered; the order, the directions, pens, sources, open strokes and every drawn segment stay as they are.  Allowed with
--no-reorder: file order, better seams.  Without the option no device call is added and every byte is what it was.

--stipple-mm (svg2stream.py's; ours as well): the plotter can lower and lift the pen on the spot (the tap, stream byte 0x03), and the stream compiler
plans such ops (orip.stream.plan_ops), but no vector front door made any.  The pass fills the shapes --hatch-fill marks with dots on one lattice for the
whole drawing, each at least --stipple-inset-mm from its shape's outline (orip_svg_stipple; include/orip.h states the rule, exact in integers on the step
grid).  It runs after the simplification and immediately before the order: the dots pass through none of dash, link, occlude, dedup, merge or simplify
(under --occlude the pass itself leaves out the dots a higher shape hides) and join the strokes as one-point ops, which the orders, --improve-order and
the pens take like any stroke; --loop-start sees a dot as the open stroke P, P.  Without the option no device call is added and every byte is what it was.

--ring-entry (ours as well): the greedy order and --allow-reverse see a closed stroke as the point its file lists first, and cross a shape to reach that
point while its outline passes under the pen.  With --ring-entry the greedy walk has every ring vertex of every closed stroke as a candidate and enters a
ring at the nearest one (orip_gcode_order_rings; include/orip.h states the rule: the same L1 key, ties to the lowest stroke and vertex; on a drawing
without a closed stroke it is the plain order).  The call stands in the place of the order; the rings are then rotated to where they were entered, so
--improve-order, --loop-start (which may still lower the travel), the plan and the preview see them there.  Greedy is not monotone: the pen-up travel is
usually lower, and nothing promises it; the tools report it.  Not with --no-reorder: file order was asked for, and --loop-start is the option for that.
Without the option no device call is added and every byte is what it was.

--arcs (ours as well): the reference's parser has no motion modes -- a line with an X or Y word is a straight move whatever G word stands in front of it --
so a G2 / G3 fillet is drawn as its chord, a full circle as nothing, and G91.1 is read as G91.  With --arcs the text goes through parse_gcode_arcs (modal
G0 .. G3, G words with their decimal, I / J and R centres, the radius rule) into a table of lines and arcs, and the arcs are flattened on the device into
the mm polylines the conversion reads without a copy (orip_gcode_flatten; include/orip.h states the rule: bisected unit vectors, no sin or cos, every point
on the circle, within --arc-tolerance-mm of it between the points; default half a step on paper).  Everything behind the conversion is unchanged.  On a
text without an arc the old parser's paths take the old route: no device call is added and every byte is what it was, as without the option."""
from __future__ import annotations

import argparse
import re
from collections import namedtuple
import sys
from dataclasses import dataclass, fields, replace
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import stream as ST

A4_MM = (210.0, 297.0)
MM_PER_INCH = 25.4
MAX_TARGET_STEPS = 1 << 30          # ours, not the reference's: step coordinates are int32 on the device


@dataclass
class GcodeOptions:
    """The command line of gcode2stream.py (:436-543): same names, same defaults."""
    output: str = "stream_from_gcode.bin"
    target_width_steps: Optional[int] = None
    target_height_steps: Optional[int] = None
    steps_per_mm: float = 40.0
    invert_y: int = 0
    offset_x_mm: float = 0.0
    offset_y_mm: float = 0.0
    scale_x: float = 1.0
    scale_y: float = 1.0
    color_index: int = 3
    div_start: int = 28
    div_fast: int = 15
    profile: str = "triangle"
    corner_deg: float = 85.0
    corner_div: int = 28
    corner_window_steps: int = 300
    travel_div_fast: int = 10
    travel_start_div: int = 28
    travel_window_steps: int = 240
    travel_quant_step: int = 4
    short_len_steps: int = 120
    short_div: int = 16
    speed_scale: float = 1.0
    no_reorder: bool = False
    allow_reverse: bool = False         # ours from here on: strokes may be drawn backwards
    tool_pens: bool = False             # T words of the text choose the pen of a path
    pen_order: Optional[str] = None     # pens in drawing order, comma-separated (default: ascending)
    merge_paths: bool = False           # strokes of one pen that meet end to end are drawn as one
    improve_order: bool = False         # 2-opt / or-opt on the order, per pen group
    improve_rounds: Optional[int] = None    # rounds per group at most (None: 2 m + 64 for a group of m strokes); only with improve_order
    clip: bool = False                  # strokes are cut at the sheet's edge (less the margin) instead of clamped to it
    clip_margin_mm: Optional[float] = None  # the clip rectangle lies this far inside the sheet (None: 0); only with clip
    simplify_mm: Optional[float] = None     # vertices within this distance of the stroke are dropped (None: every vertex is drawn; 0: only those on the stroke)
    dedup: bool = False                 # collinear segments of one pen that lie over each other are drawn once, the first drawn copy stays
    arcs: bool = False                  # G2 / G3 are drawn as arcs, flattened on the device (without it they are the reference's chords)
    arc_tolerance_mm: Optional[float] = None    # a chord leaves its arc by at most this, in the file's mm (None: half a step on paper); only with arcs
    ring_entry: bool = False            # the greedy order enters a closed stroke at its nearest ring vertex
    loop_start: bool = False            # every closed stroke starts and ends at the ring vertex that makes the pen-up travel of the plot least
    dash_mm: Optional[str] = None       # every path is drawn dashed: dash and gap lengths in mm, comma-separated (None: solid)
    dash_offset_mm: Optional[float] = None  # where in the pattern a path starts (None: 0); only with dash_mm


# ------------------------------------------------------------------ parse (:113-142, :177-300)
_COMMENT = re.compile(r"\([^)]*\)?|\)")       # "(" up to the next ")" or the end of the line, no nesting; a stray ")" goes too


def _code_lines(text: str) -> List[str]:
    out = []
    for raw in text.splitlines():
        line = _COMMENT.sub("", raw.split(";", 1)[0]).strip()
        if line:
            out.append(line)
    return out


MAX_PENS = 8


def parse_gcode(text: Union[str, bytes], pens_out: Optional[List[int]] = None) -> Tuple[np.ndarray, np.ndarray, int]:
    """Pen-down paths of a G-code text: (off int64 [n + 1], pts_mm float64 [total, 2], pen-down moves).  Path p is pts_mm[off[p]:off[p + 1]], always two
    points or more.  Words are whitespace-separated, letter + number; a word whose number does not parse is skipped whole.  G90 / G91 and G20 / G21 act
    where they stand in the line; M3 / M4 lower the pen, M5 lifts it, a Z word lowers it iff z <= 0 unless an M word of the line decided; the pen moves
    before the line's motion, and lifting it closes the path.  int(float("inf")) raises, as in the reference: such a file is refused.
    T words are skipped, as in the reference, unless a list is given as pens_out: then it receives, per path, the tool in force at the path's first
    pen-down move (-1: no T word seen so far), and a tool outside 0..7 is an error."""
    if isinstance(text, (bytes, bytearray)):
        text = bytes(text).decode("utf-8", errors="ignore")
    x = y = 0.0
    absolute, metric, down = True, True, False
    flat: List[Tuple[float, float]] = []
    off = [0]
    open_from = 0                                     # len(flat) where the open path starts (== len(flat): none open)
    moves = 0
    tool = open_tool = -1

    def close():
        nonlocal open_from
        if len(flat) - open_from >= 2:
            off.append(len(flat))
            if pens_out is not None:
                pens_out.append(open_tool)
        else:
            del flat[open_from:]
        open_from = len(flat)

    for line in _code_lines(text):
        pen = None; nx = ny = nz = None
        for word in line.split():
            letter, num = word[0].upper(), word[1:]
            if not num:
                continue
            try:
                if letter == "G" or letter == "M":
                    code = int(float(num))             # OverflowError (Ginf) is not caught: the reference fails there too
                elif letter in "XYZ":
                    v = float(num)
                elif letter == "T" and pens_out is not None:
                    code = int(float(num))
                else:
                    continue
            except ValueError:
                continue
            if letter == "T":
                if not (0 <= code < MAX_PENS):
                    raise ValueError(f"tool T{code}: the plotter has pens 0..{MAX_PENS - 1}")
                tool = code
            elif letter == "G":
                if code == 90: absolute = True
                elif code == 91: absolute = False
                elif code == 21: metric = True
                elif code == 20: metric = False
            elif letter == "M":
                if code == 3 or code == 4: pen = True
                elif code == 5: pen = False
            else:
                if not metric:
                    v *= MM_PER_INCH
                if letter == "X": nx = v
                elif letter == "Y": ny = v
                else: nz = v
        if nz is not None and pen is None:
            pen = nz <= 0.0
        if pen is not None and pen != down:
            if down:
                close()
            down = pen
        if nx is not None or ny is not None:
            ox, oy = x, y
            if absolute:
                x = nx if nx is not None else x
                y = ny if ny is not None else y
            else:
                x = x + nx if nx is not None else x
                y = y + ny if ny is not None else y
            if down:
                if len(flat) == open_from:
                    flat.append((ox, oy)); open_tool = tool
                flat.append((x, y))
                moves += 1
    close()
    return np.asarray(off, np.int64), np.asarray(flat, np.float64).reshape(-1, 2), moves


# ------------------------------------------------------------------ --arcs: the parser with motion modes (ours; the reference has none)
# What orip_gcode_flatten takes (include/orip.h): kind int32 [n_seg] (1 line, 2 arc clockwise, 3 arc counter-clockwise), seg float64 [n_seg, 6] = Ax Ay Bx By
# Cx Cy in mm, sub_off int64 [n_sub + 1]: path p is the segments sub_off[p] .. sub_off[p + 1] - 1, each starting where its predecessor ends
ArcTable = namedtuple("ArcTable", "kind seg sub_off")
ARC_LINE, ARC_CW, ARC_CCW = 1, 2, 3
ARC_STATS = ("arcs", "pieces", "full_circles")      # include/orip.h: orip_gcode_flatten
# The radius rule (ours; include/orip.h states it): the radii at the two ends may differ by 0.5 mm at most, and by more than 0.005 mm only up to a
# thousandth of the radius; an R word may be short of half the chord by 0.005 mm
ARC_RADIUS_ABS_MM, ARC_RADIUS_SMALL_MM, ARC_RADIUS_REL, ARC_R_SHORT_MM = 0.5, 0.005, 1e-3, 0.005


def parse_gcode_arcs(text: Union[str, bytes], pens_out: Optional[List[int]] = None) -> Tuple[ArcTable, int]:
    """parse_gcode with motion modes: (the segment table of the pen-down paths, pen-down moves).  Every rule of parse_gcode holds -- comments, words, G20 /
    G21, G90 / G91, the M3 / M4 / M5 and Z pen rules, T words with pens_out, how a path opens and closes -- and a pen-down move is one segment.  Added:
    G0 / G1 / G2 / G3 set the modal motion mode where they stand (the last of a line wins; G1 at the start); G words are read with their decimal, so G90.1
    (absolute centres) and G91.1 (offsets from the start point, the default) set the centre mode and leave the distance mode alone; G17 is accepted and
    after G18 / G19 an arc is an error.  In mode G2 (clockwise) / G3 a line that moves -- there also one with only I / J / R words: the end point is then
    the start point -- is an arc from the cursor A to the end point B.  I / J give the centre (a missing one: 0, resp. A's coordinate under G90.1); R
    gives the radius instead: the centre lies h = sqrt(R^2 - (d / 2)^2) from the chord's midpoint, on the left of A -> B for G3 with R > 0 and for G2
    with R < 0, otherwise on the right (R < 0: the long way round); d = 0 is an error, and so is R^2 < (d / 2)^2 unless d / 2 - |R| <= 0.005 mm (h = 0).
    I, J and R are in inches under G20.  The radii |A - C| and |B - C| must not be 0 and must agree as ARC_RADIUS_* state.  Every error is a ValueError
    naming the line.  With the pen up an arc only moves the cursor.  K, P and F are skipped."""
    if isinstance(text, (bytes, bytearray)):
        text = bytes(text).decode("utf-8", errors="ignore")
    x = y = 0.0
    absolute, metric, down, abs_centre = True, True, False, False
    mode, plane = 1, 17
    kind: List[int] = []
    seg: List[Tuple[float, float, float, float, float, float]] = []
    sub_off = [0]
    moves = 0
    tool = open_tool = -1

    def close():
        if len(kind) > sub_off[-1]:
            sub_off.append(len(kind))
            if pens_out is not None:
                pens_out.append(open_tool)

    for ln, raw in enumerate(text.splitlines(), 1):
        line = _COMMENT.sub("", raw.split(";", 1)[0]).strip()
        if not line:
            continue
        pen = None; nx = ny = nz = ni = nj = nr = None
        for word in line.split():
            letter, num = word[0].upper(), word[1:]
            if not num:
                continue
            try:
                if letter == "G":
                    code = int(round(float(num) * 10.0))   # in tenths; OverflowError (Ginf) is not caught, as in parse_gcode
                elif letter == "M":
                    code = int(float(num))
                elif letter in "XYZIJR":
                    v = float(num)
                elif letter == "T" and pens_out is not None:
                    code = int(float(num))
                else:
                    continue
            except ValueError:
                continue
            if letter == "T":
                if not (0 <= code < MAX_PENS):
                    raise ValueError(f"tool T{code}: the plotter has pens 0..{MAX_PENS - 1}")
                tool = code
            elif letter == "G":
                if code == 900: absolute = True
                elif code == 910: absolute = False
                elif code == 901: abs_centre = True
                elif code == 911: abs_centre = False
                elif code == 210: metric = True
                elif code == 200: metric = False
                elif code in (0, 10, 20, 30): mode = code // 10
                elif code in (170, 180, 190): plane = code // 10
            elif letter == "M":
                if code == 3 or code == 4: pen = True
                elif code == 5: pen = False
            else:
                if not metric:
                    v *= MM_PER_INCH
                if letter == "X": nx = v
                elif letter == "Y": ny = v
                elif letter == "Z": nz = v
                elif letter == "I": ni = v
                elif letter == "J": nj = v
                else: nr = v
        if nz is not None and pen is None:
            pen = nz <= 0.0
        if pen is not None and pen != down:
            if down:
                close()
            down = pen
        arc = mode >= 2
        if nx is None and ny is None and not (arc and (ni is not None or nj is not None or nr is not None)):
            continue
        ox, oy = x, y
        if absolute:
            x = nx if nx is not None else x
            y = ny if ny is not None else y
        else:
            x = x + nx if nx is not None else x
            y = y + ny if ny is not None else y
        cx = cy = 0.0
        if arc:
            if plane != 17:
                raise ValueError(f"line {ln}: an arc in the plane of G{plane}: only arcs in the XY plane (G17) are drawn")
            if nr is not None:
                if ni is not None or nj is not None:
                    raise ValueError(f"line {ln}: an arc with both R and I / J")
                dx, dy = x - ox, y - oy
                d = (dx * dx + dy * dy) ** 0.5
                if d == 0.0:
                    raise ValueError(f"line {ln}: an R arc whose end point is its start point has no centre")
                h2 = nr * nr - (d / 2.0) * (d / 2.0)
                if h2 < 0.0 and not (d / 2.0 - abs(nr) <= ARC_R_SHORT_MM):
                    raise ValueError(f"line {ln}: R{nr:g} mm is too short for end points {d:g} mm apart")
                if nr == 0.0 or nr != nr:
                    raise ValueError(f"line {ln}: an arc of radius R{nr:g}")
                h = h2 ** 0.5 if h2 > 0.0 else 0.0
                if (mode == 3) != (nr > 0.0):
                    h = -h                                # on the right of A -> B
                cx = (ox + x) / 2.0 + h * (-dy / d); cy = (oy + y) / 2.0 + h * (dx / d)
            elif abs_centre:
                cx = ni if ni is not None else ox; cy = nj if nj is not None else oy
            else:
                cx = ox + (ni if ni is not None else 0.0); cy = oy + (nj if nj is not None else 0.0)
            ra = ((ox - cx) ** 2 + (oy - cy) ** 2) ** 0.5; rb = ((x - cx) ** 2 + (y - cy) ** 2) ** 0.5
            if ra == 0.0 or rb == 0.0:
                raise ValueError(f"line {ln}: an arc that starts or ends on its centre")
            diff = abs(ra - rb)
            if diff > ARC_RADIUS_ABS_MM or (diff > ARC_RADIUS_SMALL_MM and diff > ra * ARC_RADIUS_REL):
                raise ValueError(f"line {ln}: the arc's radii at its start and its end, {ra:g} and {rb:g} mm, differ by {diff:g} mm")
        if down:
            if len(kind) == sub_off[-1]:
                open_tool = tool
            kind.append((ARC_CCW if mode == 3 else ARC_CW) if arc else ARC_LINE)
            seg.append((ox, oy, x, y, cx, cy))
            moves += 1
    close()
    return ArcTable(np.asarray(kind, np.int32), np.asarray(seg, np.float64).reshape(-1, 6), np.asarray(sub_off, np.int64)), moves


def arc_tolerance(o) -> Optional[float]:
    """None without --arcs, else the flattening tolerance in the file's mm (before --scale-x / --scale-y): --arc-tolerance-mm, positive and finite, or
    0.5 / (steps_per_mm max(|scale_x|, |scale_y|)), half a step on paper.  --arc-tolerance-mm belongs to --arcs."""
    t = getattr(o, "arc_tolerance_mm", None)
    if not getattr(o, "arcs", False):
        if t is not None:
            raise ValueError("--arc-tolerance-mm needs --arcs")
        return None
    if t is None:
        per_mm = float(o.steps_per_mm) * max(abs(float(o.scale_x)), abs(float(o.scale_y)))
        if not (per_mm > 0.0) or per_mm == float("inf"):
            raise ValueError("--arcs: no default tolerance when the steps per mm or both scales are 0 or not finite; give --arc-tolerance-mm")
        t = 0.5 / per_mm
    t = float(t)
    if not (t > 0.0) or t == float("inf"):
        raise ValueError("--arc-tolerance-mm must be a positive finite number")
    return t


# ------------------------------------------------------------------ options (:546-603)
def apply_speed_scale(o: GcodeOptions) -> GcodeOptions:
    """--speed-scale (:546-587): six dividers divided by the scale, rounded half to even, at least 1; then the five ordering constraints."""
    scale = float(o.speed_scale)
    if scale <= 0.0:
        raise SystemExit("Error: --speed-scale must be > 0")
    if abs(scale - 1.0) < 1e-6:
        return o
    for name in ("div_start", "div_fast", "corner_div", "short_div", "travel_div_fast", "travel_start_div"):
        setattr(o, name, max(1, int(round(getattr(o, name) / scale))))
    o.div_start = max(o.div_start, o.div_fast)
    o.corner_div = max(o.corner_div, o.div_fast)
    o.short_div = max(o.short_div, o.div_fast)
    o.travel_start_div = max(o.travel_start_div, o.travel_div_fast)
    o.div_start = max(o.div_start, o.travel_div_fast)
    return o


def target_size(o: GcodeOptions) -> Tuple[int, int]:
    """A4 at steps_per_mm unless BOTH sizes are given (:598-603)."""
    if o.target_width_steps is None or o.target_height_steps is None:
        return int(round(A4_MM[0] * o.steps_per_mm)), int(round(A4_MM[1] * o.steps_per_mm))
    return int(o.target_width_steps), int(o.target_height_steps)


def stream_config(o: GcodeOptions) -> ST.StreamConfig:
    return ST.StreamConfig(steps_per_mm=o.steps_per_mm, invert_y=bool(o.invert_y), div_start=o.div_start, div_fast=o.div_fast, profile=o.profile,
                           corner_deg=o.corner_deg, corner_div=o.corner_div, corner_window_steps=o.corner_window_steps, short_len_steps=o.short_len_steps,
                           short_div=o.short_div, travel_div_fast=o.travel_div_fast, travel_start_div=o.travel_start_div,
                           travel_window_steps=o.travel_window_steps, travel_quant_step=o.travel_quant_step)


# ------------------------------------------------------------------ emit (:399-426): orip.stream's planner over all paths
EMPTY_STREAM = bytes([ST.EOF_BYTE]) + b"\x00" * (ST.SPI_CHUNK_SIZE - 1)    # no paths: the end byte and padding, without the three leading bytes (:364-391)


def pen_sequence(pen_order: Optional[str]) -> List[int]:
    """--pen-order as the drawing sequence of all eight pens: the listed ones first, in the order given, the others behind them ascending"""
    seq: List[int] = []
    for tok in (pen_order or "").split(","):
        if not tok.strip():
            continue
        try:
            p = int(tok)
        except ValueError:
            raise ValueError(f"--pen-order: {tok.strip()!r} is not a pen number")
        if not (0 <= p < MAX_PENS) or p in seq:
            raise ValueError(f"--pen-order: pen {p} is outside 0..{MAX_PENS - 1} or listed twice")
        seq.append(p)
    return seq + [p for p in range(MAX_PENS) if p not in seq]


def path_ends(off: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """(first x, first y, last x, last y) of every path: int32 [n, 4], what the orders and the improvement take"""
    return np.ascontiguousarray(np.concatenate([pts[off[:-1]], pts[off[1:] - 1]], 1), np.int32)


def gather_paths(off: np.ndarray, pts: np.ndarray, order: np.ndarray, rev: Optional[np.ndarray] = None, seam: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """the paths in the given order, those with rev[k] set back to front: (off, pts), flat numpy over all paths.  seam[k] > 0 (by position, closed strokes
    only: include/orip.h, orip_gcode_seam): the stroke of L points is rotated to start and end at its stored vertex seam[k], s, s + 1, .., L - 2, 0, .., s,
    before rev turns it round.  A one-point op (a dot of --stipple-mm) has no seam and stays as it is"""
    order = np.asarray(order, np.int64)
    lens = np.diff(off)[order]
    noff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    t = np.arange(int(lens.sum())) - np.repeat(noff[:-1], lens)
    if rev is not None:
        t = np.where(np.repeat(np.asarray(rev, bool), lens), np.repeat(lens, lens) - 1 - t, t)
    if seam is not None:
        s = np.repeat(np.asarray(seam, np.int64), lens)
        t = np.where(s > 0, (t + s) % np.repeat(np.maximum(lens - 1, 1), lens), t)
    return noff, pts[np.repeat(off[:-1][order], lens) + t]


def plan_pens(off: np.ndarray, pts: np.ndarray, path_pen: np.ndarray, head: Sequence[int], sc: ST.StreamConfig, is_tap: Optional[np.ndarray] = None) -> ST.Plan:
    """The plan of paths in drawing order whose pens come in runs (path_pen[k]: the pen of path k), from (0, 0): the service bytes `head`, then per run
    what draw_color_group does (:317-333) -- the approach to the run's first point when the cursor is elsewhere, the colour byte, and per path a travel
    when the cursor is elsewhere, pen down, the segments, pen up.  The pattern of orip.stream.plan_layers, every move by the same engine.  is_tap[k]: path
    k is one point and is drawn as a tap (None: no path is)."""
    off = np.asarray(off, np.int64); pts = np.asarray(pts, np.int64).reshape(-1, 2); path_pen = np.asarray(path_pen, np.int64)
    is_tap = np.zeros(len(path_pen), bool) if is_tap is None else np.asarray(is_tap, bool)
    plans = [ST.fixed_plan(list(head))]
    cur = np.zeros(2, np.int64)
    cuts = np.concatenate([[0], np.nonzero(np.diff(path_pen))[0] + 1, [len(path_pen)]]) if len(path_pen) else np.zeros(1, np.int64)
    for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        pen = int(path_pen[a])
        if not (0 <= pen < MAX_PENS):
            raise ValueError("color index 0..7")
        goff, gpts = off[a:b + 1] - off[a], pts[off[a]:off[b]]
        if (cur != gpts[0]).any():
            plans.append(ST.fixed_plan([-1], [[*cur, *gpts[0]]])); cur = gpts[0]
        plans.append(ST.plan_ops(goff, gpts, is_tap[a:b], cur, [0x08 | pen], False, sc))
        cur = gpts[-1]
    return ST.concat_plans(plans)


def build_stream_from_gcode(text_or_paths, opts: Optional[GcodeOptions] = None, device=None, *, steps_fn: Optional[Callable] = None,
                            order_fn: Optional[Callable] = None, codes_fn: Optional[Callable] = None, pack_fn: Optional[Callable] = None,
                            timings: Optional[dict] = None, pens: Optional[np.ndarray] = None, order_pens_fn: Optional[Callable] = None,
                            source_fn: Optional[Callable] = None, merge_fn: Optional[Callable] = None, improve_fn: Optional[Callable] = None,
                            clip_fn: Optional[Callable] = None, simplify_fn: Optional[Callable] = None, dedup_fn: Optional[Callable] = None,
                            dash_fn: Optional[Callable] = None, seam_fn: Optional[Callable] = None, ring_entry_fn: Optional[Callable] = None,
                            flatten_fn: Optional[Callable] = None) -> Tuple[bytes, dict]:
    """The stream of a G-code text (str / bytes) or of paths in mm given as (off, pts_mm); opts as parsed, --speed-scale not yet applied.
    Device steps, each None = the GPU (orip.device.Device; there is no CPU path in the product).  PASSES below states every signature and the place of
    every pass; here, which option asks for which step and what it leaves in info:
      steps_fn, order_fn, codes_fn, pack_fn   always (codes_fn and pack_fn: orip.stream.compile_plan)
      source_fn, order_pens_fn   only with pens or --allow-reverse
      merge_fn        only with --merge-paths.  info["merge"] holds paths_in, paths_out, joins and cycles; the pen of a merged path is its members' pen.
      improve_fn      only with --improve-order (without pens: one group, no stroke reversed).  info["improve"] holds travel_before, travel_after (pen-up
                      steps of the whole plot), rounds, converged_groups and skipped_groups.
      clip_fn         only with --clip, in the place of steps_fn (source_fn keeps its meaning: the input path of every stroke, now with repeats).
                      info["clip"] holds rect and segments, inside, cut, outside, paths_out and points_out.
      simplify_fn     only with --simplify-mm.  info["simplify"] holds tol4, points_in, points_out and paths_changed.
      dedup_fn        only with --dedup.  info["dedup"] holds segments, whole, cut, covered, pieces, paths_out, points_out, draw_steps_in and draw_steps_out;
                      a stroke keeps its origin's pen.
      dash_fn         only with --dash-mm (it needs source_fn).  info["dash"] holds the eight counts of include/orip.h; a dash keeps its stroke's pen.
      seam_fn         only with --loop-start.  info["seam"] holds closed, moved, travel_before and travel_after (pen-up steps of the whole plot).
      ring_entry_fn   only with --ring-entry, in the place of order_fn / order_pens_fn (without pens: one group).  info["ring_entry"] holds closed, moved,
                      candidates and travel (pen-up steps of the sequence as the call returned it).
      flatten_fn      only with --arcs on a text that holds a G2 / G3 arc (parse_gcode_arcs then stands in parse_gcode's place).  info["arcs"] holds
                      tolerance_mm, arcs, pieces and full_circles.  On a text without an arc the option changes nothing: parse_gcode's paths, no
                      flatten_fn call, the same bytes.
    pens: one pen per input path, 0..7, or -1 for --color-index (a text's T words under --tool-pens when None).  info["pens"] then counts the paths per
    pen, those that took --color-index ("unmatched") and the strokes drawn backwards ("reversed").
    Returns (bytes, counts)."""
    fn = dict(flatten=flatten_fn, convert=clip_fn if opts is not None and opts.clip else steps_fn, dash=dash_fn, dedup=dedup_fn, merge=merge_fn, simplify=simplify_fn,
              order=order_fn, order_pens=order_pens_fn, ring_entry=ring_entry_fn, improve=improve_fn, seam=seam_fn, source=source_fn, codes=codes_fn, pack=pack_fn)
    return stroke_stream(text_or_paths, opts, device, StrokeSteps(fn), timings, pens)


# ------------------------------------------------------------------ the stroke driver: what a pass is, stated once
# One row per pass, in pipeline order.  keywords: the step keywords of the front doors that give a stand-in for the device's pass (the SVG door takes all,
# the G-code door all but SVG_ONLY_STEPS); info, timing: the keys the pass writes to info and to `timings`; rewrites: the pass leaves a new stroke list,
# on a device as its resident step polylines; method: the orip.device.Device method of the uploaded form; resident: the driver also calls the pass in a
# form that reads the list the device holds (resolve_steps says when).  A stand-in is called as the device's uploaded form is, and returns what it returns:
#   flatten     fn(table: ArcTable, tol) -> (off int64, pts_mm float64 [total, 2], stats), or (None, None, stats): the polylines stay resident for this
#               device's own conversion, which is then called as convert(None, None, map[, rect], n=paths).  In front of the conversion
#   convert     steps_fn(off, pts_mm, map: dict) -> (off int64, pts int32 [total, 2]); with --clip, in its place,
#               clip_fn(off, pts_mm, map, rect: (x0, y0, x1, y1)) -> (off, pts, stats)
#   dash        fn(off, pts, pattern int32 [n], phase int64 [n], pat_off, pat_val) -> (off, pts, origin int32: the input stroke of every output stroke,
#               stats).  Behind the pens of the strokes, before the occlusion: a shape on top cuts dashes as it does on a screen
#   hatch_link  fn(off, pts, cls int32 [n], ring_sub, ring_group, map, clamp, reach) -> (off, pts, member_off int64, member int32: the input strokes of
#               every output stroke, stats).  Before the occlusion: it sees the hatch lines whole, and a shape on top cuts a zigzag
#   occlude     fn(off, pts, level int32 [n], ring_sub, ring_level, map, clamp) -> (off, pts, origin int32, stats)
#   dedup       fn(off, pts, group int32 [n], n_groups) -> (off, pts, origin int32, stats).  Before the merge, which joins the pieces it leaves
#   merge       fn(off, pts, group int32 [n], n_groups, reverse) -> (off, pts, member_off, member, rev, counts)
#   simplify    fn(off, pts, tol4) -> (off, pts, kept int64: the input index of every output point, stats).  Behind the merge: the joints can go
#   stipple     fn(ring_sub, ring_group, map, clamp, lattice, inset, rect, flags) -> (xy int32 [dots, 2], group int32 [dots], stats).  It touches no
#               stroke; its dots join the strokes as one-point ops immediately before the order
#   order       order_fn(ends int32 [n, 4]) -> order int32 [n], or with pens or --allow-reverse
#               order_pens_fn(ends, group int32 [n], n_groups, reverse) -> (order, rev)
#   ring_entry  fn(off, pts, group int32 [n], n_groups, reverse) -> (order int32 [n], rev bool [n], seam int32 [n]: by sequence position, the stored ring
#               vertex a closed stroke is entered at, 0 for an open one; stats).  --ring-entry, in the place of the order
#   improve     fn(ends, group int32 [n], n_groups, order, rev, reverse, max_rounds) -> (order, rev, stats).  Behind the order
#   seam        fn(off, pts, order int32 [n] or None, rev bool [n] or None) -> (seam int32 [n] by sequence position, stats).  Behind the order and the
#               improvement, immediately before the paths are gathered
# In the SVG door's keywords the fitted paths stand in front of the arguments of convert (in the place of off, pts_mm), hatch_link, occlude and stipple
# (orip.svg.build_stream_from_svg).  source_fn(n) -> src int32 [n], the input path of every step polyline (orip_gcode_steps_source_fetch), is no pass.
Pass = namedtuple("Pass", "name keywords info timing rewrites method resident")
PASSES = (
    Pass("flatten", ("flatten_fn",), "arcs", "flatten", False, "gcode_flatten", False),
    Pass("convert", ("steps_fn", "clip_fn"), "clip", "to_steps", True, "gcode_to_steps", True),
    Pass("dash", ("dash_fn",), "dash", "dash", True, "gcode_dash", True),
    Pass("hatch_link", ("hatch_link_fn",), "hatch_link", "hatch_link", True, "gcode_hatch_link", True),
    Pass("occlude", ("occlude_fn",), "occlude", "occlude", True, "gcode_occlude", True),
    Pass("dedup", ("dedup_fn",), "dedup", "dedup", True, "gcode_dedup", True),
    Pass("merge", ("merge_fn",), "merge", "merge", True, "gcode_merge", True),
    Pass("simplify", ("simplify_fn",), "simplify", "simplify", True, "gcode_simplify", True),
    Pass("stipple", ("stipple_fn",), "stipple", "stipple", False, "svg_stipple", False),
    Pass("order", ("order_fn", "order_pens_fn"), None, "order", False, "gcode_order", False),
    Pass("ring_entry", ("ring_entry_fn",), "ring_entry", "order", False, "gcode_order_rings", True),
    Pass("improve", ("improve_fn",), "improve", "improve", False, "gcode_improve", False),
    Pass("seam", ("seam_fn",), "seam", "seam", False, "gcode_seam", True),
)
SVG_ONLY_STEPS = ("hatch_link_fn", "occlude_fn", "stipple_fn")
OTHER_STEPS = ("source_fn", "codes_fn", "pack_fn")              # step keywords of both doors that are no pass


def _flat(v, dtype):
    return np.asarray(v, dtype).reshape(-1)


# The per-drawing data of the four passes that take some.  A stroke takes its entry of a path_* table through its source.
class Dash(namedtuple("Dash", "path_pattern path_phase pat_off pat_val")):
    """--dash-mm here, --dashes of the SVG door: pattern (-1: solid) and phase of every input path; the pattern table in 1/256 step (include/orip.h)"""
    def __new__(cls, path_pattern, path_phase, pat_off, pat_val):
        return super().__new__(cls, _flat(path_pattern, np.int32), _flat(path_phase, np.int64), _flat(pat_off, np.int32), _flat(pat_val, np.int64))


class Occlude(namedtuple("Occlude", "path_level ring_sub ring_level clamp")):
    """--occlude of the SVG door: the level of every input path; the rings as fitted paths and their levels; clamp = the rings are clamped as the strokes were"""
    def __new__(cls, path_level, ring_sub, ring_level, clamp):
        return super().__new__(cls, _flat(path_level, np.int64), _flat(ring_sub, np.int32), _flat(ring_level, np.int32), bool(clamp))


class HatchLink(namedtuple("HatchLink", "path_cls ring_sub ring_group clamp reach")):
    """--hatch-connect of the SVG door: the class 2 g + f of every input path (-1: no hatch line); the rings as fitted paths and the shape g of each; clamp
    as Occlude's; reach = the longest link in steps (include/orip.h)"""
    def __new__(cls, path_cls, ring_sub, ring_group, clamp, reach):
        return super().__new__(cls, _flat(path_cls, np.int64), _flat(ring_sub, np.int32), _flat(ring_group, np.int32), bool(clamp), int(reach))


class Stipple(namedtuple("Stipple", "ring_sub ring_group clamp lattice inset rect flags pen_of")):
    """--stipple-mm of the SVG door: the rings as HatchLink's; lattice = (pitch, row, shift) and inset in steps; rect = (x0, y0, x1, y1), the sheet or the
    clip rectangle; flags of STIPPLE_SERPENTINE and STIPPLE_OCCLUDE; pen_of(group int64 [dots]) -> the pen of every dot, -1 for --color-index (None:
    every dot takes --color-index)"""
    def __new__(cls, ring_sub, ring_group, clamp, lattice, inset, rect, flags, pen_of=None):
        return super().__new__(cls, _flat(ring_sub, np.int32), _flat(ring_group, np.int32), bool(clamp), tuple(int(v) for v in lattice), int(inset),
                               tuple(int(v) for v in rect), int(flags), pen_of)


@dataclass(frozen=True)
class StrokeSteps:
    """The passes of one drawing: fn[name] for the rows of PASSES and for "order_pens", "source", "codes" and "pack" (absent or None: not given); the data of
    the passes that take some (None: the pass does not run); own: the names resolve_steps filled from its device"""
    fn: dict
    dash: Optional[Dash] = None
    hatch_link: Optional[HatchLink] = None
    occlude: Optional[Occlude] = None
    stipple: Optional[Stipple] = None
    own: frozenset = frozenset()


def steps_needed(st: StrokeSteps, o, grouped: bool, flatten: bool = False) -> List[str]:
    """the names in st.fn this drawing calls for: the passes that are on, in the order of PASSES, then "order_pens" and "source".  flatten: --arcs found an arc"""
    ring = bool(o.ring_entry)
    on = dict(flatten=flatten, convert=True, dash=st.dash is not None, hatch_link=st.hatch_link is not None, occlude=st.occlude is not None, dedup=bool(o.dedup),
              merge=bool(o.merge_paths), simplify=o.simplify_mm is not None, stipple=st.stipple is not None, order=not ring, ring_entry=ring,
              improve=bool(o.improve_order), seam=bool(o.loop_start))
    sources = bool(grouped) or on["dash"] or on["hatch_link"] or on["occlude"]
    return [p.name for p in PASSES if on[p.name]] + ["order_pens"] * (bool(grouped) and not ring) + ["source"] * sources


def _resident_form(method):
    """a device's pass, called with the strokes the host holds, run on the list the device holds: every resident-form call is this one"""
    return lambda off, pts, *a: method(None, None, *a, n=len(off) - 1)


def _ring_pass(upload, run, resident: bool):
    """a device's occlusion or hatch link.  Its rings are fitted paths, which only the svg_* form `run` reads, and that form has no uploaded one: behind a
    given pass the strokes are uploaded first, through the ring-less gcode_* form `upload`, which makes them the resident list"""
    def call(off, pts, key, ring_sub, ring_key, m, clamp, *reach):
        if not resident:
            upload(off, pts, key, np.zeros(1, np.int64), np.zeros((0, 2), np.int32), np.zeros(0, np.int32), *reach)
        return run(key, ring_sub, ring_key, m, clamp, *reach, n=len(off) - 1)
    return call


def _own_flatten(device, resident: bool):
    """a device's flattening: the polylines stay resident for its own conversion and are fetched for a given one"""
    def call(table, tol):
        _total, stats = device.gcode_flatten(table, tol)
        return (None, None, stats) if resident else (*device.svg_paths(), stats)
    return call


def _own_improve(method):
    return lambda ends, group, n_groups, order, rev, reverse, max_rounds: method(ends, group, n_groups, order, rev, reverse, max_rounds=max_rounds)


def resolve_steps(st: StrokeSteps, o, grouped: bool, device=None, convert: Optional[Callable] = None, force: bool = False, flatten: bool = False):
    """The steps the drawing needs (steps_needed), those not given taken from a device -> (steps, device); codes and pack stay as given
    (orip.stream.compile_plan fills them).  When none is missing, and the caller does not `force` a device for steps of its own, no device is made and
    orip.stages is not imported.  convert(device) -> the conversion of a front door whose paths are on the device already (orip.svg).

    THE RESIDENCY RULE.  The table is walked in order.  An own pass that has a resident form reads the resident list iff the last list-rewriting pass that
    ran was this device's own; otherwise it is sent its input.  The exceptions, each stated here and nowhere else:
      - with a stipple the ring order and the seam pass are always sent their strokes: the dots among them are in no resident list;
      - behind a ring order, which rotates the rings on the host, the seam pass is always sent its strokes;
      - occlude and hatch link have no uploaded form that reads their rings: _ring_pass;
      - the flattening returns (None, None, stats) only in front of this device's own conversion, and fetches its polylines for a given one."""
    need = steps_needed(st, o, grouped, flatten)
    if not force and all(st.fn.get(k) is not None for k in need):
        return st, device
    if device is None:
        from .stages import device as _default_device
        device = _default_device()
    fn = {k: st.fn.get(k) for k in need + ["codes", "pack"]}
    own = {k for k in need if fn[k] is None}
    dots, ring = st.stipple is not None, "ring_entry" in need
    resident = False                                    # the last list-rewriting pass that ran was this device's own
    for p in PASSES:
        if p.name not in need:
            continue
        if p.name in own:
            method, reads = getattr(device, p.method), p.resident and resident
            if p.name == "flatten":
                fn[p.name] = _own_flatten(device, "convert" in own)
            elif p.name == "convert":                   # its resident form reads the flattened paths: _convert asks for it with n=
                fn[p.name] = convert(device) if convert is not None else device.gcode_to_steps_clip if o.clip else method
            elif p.name in ("hatch_link", "occlude"):
                fn[p.name] = _ring_pass(method, getattr(device, "svg_" + p.name), reads)
            elif p.name == "improve":
                fn[p.name] = _own_improve(method)
            else:
                reads = reads and not (dots and p.name in ("ring_entry", "seam")) and not (ring and p.name == "seam")
                fn[p.name] = _resident_form(method) if reads else method
        if p.rewrites:
            resident = p.name in own
    for name, method in (("order_pens", device.gcode_order_pens), ("source", device.gcode_steps_source)):
        if name in own:
            fn[name] = method
    return replace(st, fn=fn, own=frozenset(own)), device


def _host_sources(st: StrokeSteps, name: str, what: str, src) -> StrokeSteps:
    """The sources behind the dash pass and the hatch link (`name`), which both change the stroke list in front of a pass that asks for them.  A device's
    sources follow its own passes, through origin resp. through a zigzag's first line; unless both the pass and `source` are this device's, the host has
    gathered them the same way (`src`, which _dash and _hatch_link hand over) and they are the source step from here on"""
    if name in st.own and "source" in st.own:
        return st

    def gathered(n):
        if n != len(src):
            raise RuntimeError(f"{n} sources asked for, {what} left {len(src)} strokes")
        return src
    return replace(st, fn=dict(st.fn, source=gathered), own=st.own - {"source"})


def _convert(st: StrokeSteps, off_mm, pts_mm, m: dict, rect, info: dict, n_resident: Optional[int] = None):
    """mm paths -> step polylines, clamped to the sheet or (rect) cut at it; info["clip"].  n_resident: the paths are that many the flattening left on the device"""
    more = {} if n_resident is None else {"n": int(n_resident)}
    if rect is None:
        off, pts = st.fn["convert"](off_mm, pts_mm, m, **more)
    else:
        off, pts, cst = st.fn["convert"](off_mm, pts_mm, m, rect, **more)
        info["clip"] = dict({"rect": tuple(int(v) for v in rect)}, **{k: int(cst[k]) for k in CLIP_STATS})
        if info["clip"]["inside"] + info["clip"]["cut"] + info["clip"]["outside"] != info["clip"]["segments"] or info["clip"]["paths_out"] != len(off) - 1:
            raise RuntimeError("the clip's counts do not add up")
    return np.asarray(off, np.int64), np.asarray(pts, np.int32).reshape(-1, 2)


def _sources(st: StrokeSteps, n: int, n_paths: int, tables_ok: bool = True):
    """the input path of each of the n step polylines, checked against the n_paths input paths (tables_ok: the caller's per-path tables are of one length)"""
    src = np.asarray(st.fn["source"](n), np.int64).reshape(-1)
    if len(src) != n or (src < 0).any() or (src >= n_paths).any() or not tables_ok:
        raise RuntimeError("the source indices of the step polylines do not name input paths")
    return src


def _cut_result(what: str, out, n_in: int, pen, group, info: dict, may_be_empty: bool = True):
    """What a cutting pass (`what`: "the dedup", "the occlusion", "the dash pass") returned, (off, pts, origin), normalised and checked: the origins are the
    input strokes in ascending order, every stroke has two points or more and no repeated point, and at least one is left unless the pass may leave none.
    Pen and group follow origin; info["paths"].  -> (off, pts, origin, pen, group)"""
    off, pts, origin = out
    off = np.asarray(off, np.int64).reshape(-1); pts = np.asarray(pts, np.int32).reshape(-1, 2); origin = np.asarray(origin, np.int64).reshape(-1)
    n = len(off) - 1
    if n < (0 if may_be_empty else 1) or len(origin) != n or (np.diff(origin) < 0).any() or (n and (origin[0] < 0 or origin[-1] >= n_in)):
        raise RuntimeError(f"{what}'s origins are not the input strokes in ascending order")
    same = (np.diff(pts, axis=0) == 0).all(1) if len(pts) > 1 else np.zeros(0, bool)
    if off[0] != 0 or int(off[-1]) != len(pts) or (np.diff(off) < 2).any() or np.delete(same, off[1:-1] - 1).any():
        raise RuntimeError(f"{what} returned a stroke of fewer than two points or with a repeated point")
    if group is not None:
        pen, group = pen[origin], group[origin]
    info["paths"] = n
    return off, pts, origin, pen, group


def _stroke_pens(st: StrokeSteps, o: GcodeOptions, pens, n: int, info: dict):
    """(pen, group) of every step polyline: its input path's pen, through the paths the conversion dropped, and that pen's place in the drawing sequence"""
    if not (0 <= int(o.color_index) <= 7):
        raise ValueError("color index 0..7")
    if pens is None:
        return np.full(n, int(o.color_index), np.int64), np.zeros(n, np.int32)
    src = _sources(st, n, len(pens))
    pen = np.where(pens[src] < 0, int(o.color_index), pens[src])
    info["pens"] = {"paths": np.bincount(pen, minlength=MAX_PENS).tolist(), "unmatched": int((pens[src] < 0).sum()), "reversed": 0}
    return pen, np.argsort(np.asarray(pen_sequence(o.pen_order)))[pen].astype(np.int32)


def _merge(st: StrokeSteps, o: GcodeOptions, off, pts, pen, group, n_groups: int, info: dict):
    """strokes of one pen that meet end to end become one; the pen of a merged stroke is its members' pen; info["merge"]"""
    n_in = len(off) - 1
    off, pts, member_off, member, _, mst = st.fn["merge"](off, pts, group if group is not None else np.zeros(n_in, np.int32), n_groups, bool(o.allow_reverse))
    off = np.asarray(off, np.int64); pts = np.asarray(pts, np.int32).reshape(-1, 2)
    member_off = np.asarray(member_off, np.int64).reshape(-1); member = np.asarray(member, np.int64).reshape(-1)
    n = len(off) - 1
    if not (1 <= n <= n_in) or len(member_off) != n + 1 or len(member) != n_in or int(member_off[-1]) != n_in or not np.array_equal(np.sort(member), np.arange(n_in)):
        raise RuntimeError("the merge did not return every path once")
    if group is not None:
        first = member[member_off[:-1]]
        if (group[member] != np.repeat(group[first], np.diff(member_off))).any():
            raise RuntimeError("the merge joined paths of different pens")
        pen, group = pen[first], group[first]
    info["paths"] = n
    info["merge"] = {"paths_in": n_in, "paths_out": n, "joins": int(mst["joins"]), "cycles": int(mst["cycles"])}
    return off, pts, pen, group


def draw_steps(off, pts) -> int:
    """the pen-down steps of the strokes as the stream compiler counts them: max(|dx|, |dy|) per segment"""
    d = np.abs(np.diff(np.asarray(pts, np.int64).reshape(-1, 2), axis=0)).max(1) if len(pts) > 1 else np.zeros(0, np.int64)
    inner = np.ones(len(d), bool); inner[np.asarray(off[1:-1], np.int64) - 1] = False          # the gap between two strokes is not a segment
    return int(d[inner].sum())


def _dedup(st: StrokeSteps, off_in, pts_in, pen, group, n_groups: int, info: dict):
    """the strokes less every stretch an earlier segment of the same pen has drawn; a stroke left in parts keeps its pen; info["dedup"]"""
    n_in = len(off_in) - 1
    *out, dst = st.fn["dedup"](off_in, pts_in, group if group is not None else np.zeros(n_in, np.int32), n_groups)
    d = {k: int(dst[k]) for k in DEDUP_STATS}
    off, pts, origin, pen, group = _cut_result("the dedup", out, n_in, pen, group, info, may_be_empty=False)
    n = len(off) - 1
    if d["whole"] + d["cut"] + d["covered"] != d["segments"] or d["segments"] != len(pts_in) - n_in or d["paths_out"] != n or d["points_out"] != len(pts) or \
            d["pieces"] != len(pts) - n or d["pieces"] > 2 * d["segments"] or d["draw_steps_in"] != draw_steps(off_in, pts_in) or d["draw_steps_out"] != draw_steps(off, pts):
        raise RuntimeError("the dedup's counts do not add up")
    if d["draw_steps_out"] > d["draw_steps_in"]:
        raise RuntimeError("the dedup added ink")
    info["dedup"] = d
    return off, pts, pen, group


def _occlude(st: StrokeSteps, off_in, pts_in, pen, group, m: dict, info: dict):
    """the strokes less what a shape of a higher level hides; a stroke takes its level through its source, and what is left of it keeps its pen; info["occlude"]"""
    oc, n_in = st.occlude, len(off_in) - 1
    src = _sources(st, n_in, len(oc.path_level))
    *out, ost = st.fn["occlude"](off_in, pts_in, oc.path_level[src].astype(np.int32), oc.ring_sub, oc.ring_level, m, oc.clamp)
    d = {k: int(ost[k]) for k in OCCLUDE_STATS}
    off, pts, origin, pen, group = _cut_result("the occlusion", out, n_in, pen, group, info)
    n = len(off) - 1
    if d["whole"] + d["cut"] + d["hidden"] != d["segments"] or d["segments"] != len(pts_in) - n_in or d["paths_out"] != n or d["points_out"] != len(pts) or \
            d["pieces"] - d["collapsed"] != len(pts) - n or d["draw_steps_in"] != draw_steps(off_in, pts_in) or d["draw_steps_out"] != draw_steps(off, pts):
        raise RuntimeError("the occlusion's counts do not add up")
    info["occlude"] = d
    return off, pts, pen, group


def _dash(st: StrokeSteps, off_in, pts_in, pen, group, info: dict):
    """the strokes, those with a pattern as their dashes; a stroke takes pattern and phase through its source, and a dash keeps its stroke's pen and, the
    source (_host_sources: the steps with them are the first value returned); info["dash"]"""
    dh, n_in = st.dash, len(off_in) - 1
    src = _sources(st, n_in, len(dh.path_pattern), len(dh.path_phase) == len(dh.path_pattern))
    pattern = dh.path_pattern[src]
    *out, dst = st.fn["dash"](off_in, pts_in, pattern, dh.path_phase[src], dh.pat_off, dh.pat_val)
    d = {k: int(dst[k]) for k in DASH_STATS}
    off, pts, origin, pen, group = _cut_result("the dash pass", out, n_in, pen, group, info)
    n = len(off) - 1
    if d["paths_in"] != n_in or d["dashed"] != int((pattern >= 0).sum()) or d["paths_out"] != n or d["points_out"] != len(pts) or \
            d["paths_out"] != d["paths_in"] - d["dashed"] + d["dashes"] - d["collapsed"] or not (0 <= d["length_on"] <= d["length_in"]):
        raise RuntimeError("the dash pass's counts do not add up")
    info["dash"] = d
    return _host_sources(st, "dash", "the dash pass", src[origin]), off, pts, pen, group


def _hatch_link(st: StrokeSteps, off_in, pts_in, pen, group, m: dict, info: dict):
    """the strokes, the hatch lines joined into zigzags; a stroke takes its class through its source, and a zigzag keeps the pen and the source of its
    first line (_host_sources: the steps with them are the first value returned); info["hatch_link"]"""
    hl, n_in = st.hatch_link, len(off_in) - 1
    src = _sources(st, n_in, len(hl.path_cls))
    cls = hl.path_cls[src]
    off, pts, member_off, member, lst = st.fn["hatch_link"](off_in, pts_in, cls.astype(np.int32), hl.ring_sub, hl.ring_group, m, hl.clamp, hl.reach)
    off = np.asarray(off, np.int64).reshape(-1); pts = np.asarray(pts, np.int32).reshape(-1, 2)
    member_off = np.asarray(member_off, np.int64).reshape(-1); member = np.asarray(member, np.int64).reshape(-1)
    d = {k: int(lst[k]) for k in HATCH_LINK_STATS}
    n = len(off) - 1
    if not (1 <= n <= n_in) or len(member_off) != n + 1 or len(member) != n_in or member_off[0] != 0 or int(member_off[-1]) != n_in or (np.diff(member_off) < 1).any() or \
            not np.array_equal(np.sort(member), np.arange(n_in)):
        raise RuntimeError("the hatch link did not return every stroke once")
    first = member[member_off[:-1]]
    lens = np.diff(member_off)
    if (np.diff(first) <= 0).any() or (cls[member] != np.repeat(cls[first], lens)).any() or (cls[first][lens > 1] < 0).any() or \
            (group is not None and (group[member] != np.repeat(group[first], lens)).any()):
        raise RuntimeError("the hatch link joined strokes of different shapes or pens, or left them out of order")
    if off[0] != 0 or int(off[-1]) != len(pts) or (np.diff(off) < 2).any() or d["paths_out"] != n or n != n_in - d["links"] or d["points_out"] != len(pts) or \
            len(pts) != len(pts_in) - d["coincident"] or d["lines"] != int(((cls >= 0) & (np.diff(off_in) == 2)).sum()) or not (d["links"] <= d["eligible"] <= d["in_reach"]) or \
            draw_steps(off, pts) != draw_steps(off_in, pts_in) + d["link_steps"]:
        raise RuntimeError("the hatch link's counts do not add up")
    if group is not None:
        pen, group = pen[first], group[first]
    info["paths"] = n
    info["hatch_link"] = dict(d, reach=hl.reach)
    return _host_sources(st, "hatch_link", "the hatch link", src[first]), off, pts, pen, group




def _simplify(st: StrokeSteps, off_in, pts_in, tol4: int, info: dict):
    """the same strokes with the same ends, every stroke an ascending selection of its own points; info["simplify"]"""
    n = len(off_in) - 1
    off, pts, kept, _ = st.fn["simplify"](off_in, pts_in, tol4)
    off = np.asarray(off, np.int64).reshape(-1); pts = np.asarray(pts, np.int32).reshape(-1, 2); kept = np.asarray(kept, np.int64).reshape(-1)
    if len(off) != n + 1 or off[0] != 0 or int(off[-1]) != len(pts) or len(kept) != len(pts) or (np.diff(off) < 2).any() or \
            not np.array_equal(kept[off[:-1]], off_in[:-1]) or not np.array_equal(kept[off[1:] - 1], off_in[1:] - 1) or \
            (np.diff(kept) <= 0).any() or not np.array_equal(pts, pts_in[kept]):
        raise RuntimeError("the simplification did not return every stroke with its ends and its points in order")
    info["simplify"] = {"tol4": tol4, "points_in": len(pts_in), "points_out": len(pts), "paths_changed": int((np.diff(off) != np.diff(off_in)).sum())}
    return off, pts


def _checked_order(order, rev, n: int, group, reverse: bool, what: str):
    """(order int64, rev bool) when order is a permutation of the n strokes whose groups do not decrease and nothing is reversed without `reverse`"""
    order = np.asarray(order, np.int64).reshape(-1)
    rev = np.zeros(n, bool) if rev is None else np.asarray(rev, bool).reshape(-1)
    if len(order) != n or len(rev) != n or not np.array_equal(np.sort(order), np.arange(n)) or (np.diff(np.asarray(group)[order]) < 0).any() or (rev.any() and not reverse):
        raise RuntimeError(what)
    return order, rev


def _ring_entry(st: StrokeSteps, o: GcodeOptions, off, pts, group, n_groups: int, info: dict):
    """--ring-entry: the greedy sequence with every closed stroke entered at its nearest ring vertex -> (pts with every ring rotated in place to the vertex
    it was entered at, (order, rev)); info["ring_entry"].  Checked as _checked_order checks, and: the seams name a ring vertex of every closed stroke and are
    0 elsewhere, no closed stroke is reversed, the counts add up and the travel is that of the strokes as gathered"""
    n = len(off) - 1
    grp = np.zeros(n, np.int32) if group is None else np.asarray(group, np.int32)
    order, rev, seam, rst = st.fn["ring_entry"](off, pts, grp, n_groups if group is not None else 1, bool(o.allow_reverse))
    order, rev = _checked_order(order, rev, n, grp, bool(o.allow_reverse), "the ring order is not a permutation that keeps the pens together and the directions allowed")
    seam = np.asarray(seam, np.int64).reshape(-1)
    d = {k: int(rst[k]) for k in RING_ENTRY_STATS}
    lens = np.diff(off)[order]
    closed = (lens >= 4) & (pts[off[:-1][order]] == pts[off[1:][order] - 1]).all(1)
    if len(seam) != n or (seam < 0).any() or (seam[~closed] != 0).any() or (seam[closed] >= lens[closed] - 1).any() or rev[closed].any():
        raise RuntimeError("the ring order's seams do not name a ring vertex of every closed stroke, forwards, and 0 for every open one")
    candidates = int(np.where(closed, lens - 1, 1 + bool(o.allow_reverse)).sum())
    if d["closed"] != int(closed.sum()) or d["moved"] != int((seam != 0).sum()) or d["candidates"] != candidates or \
            d["travel"] != travel_steps(*gather_paths(off, pts, order, rev, seam)):
        raise RuntimeError("the ring order's counts do not add up")
    info["ring_entry"] = d
    by_stroke = np.zeros(n, np.int64); by_stroke[order] = seam
    return gather_paths(off, pts, np.arange(n), None, by_stroke)[1], (order, rev)


def _order(st: StrokeSteps, o: GcodeOptions, off, pts, group, n_groups: int, info: dict, lap, greedy=None):
    """the drawing sequence (order, rev), or (None, None) for the strokes as they stand: pen after pen (group given) or as one list, greedy and then improved.
    greedy: the checked sequence --ring-entry has found already, in the place of either greedy order"""
    n = len(off) - 1
    if o.no_reorder:                                                      # pen after pen all the same, file order inside a pen
        return (np.argsort(group, kind="stable"), np.zeros(n, bool)) if group is not None else (None, None)
    ends, reverse = path_ends(off, pts), bool(o.allow_reverse)
    if greedy is not None:
        order, rev = greedy
        if group is None:
            group, n_groups = np.zeros(n, np.int32), 1
    elif group is not None:
        order, rev = _checked_order(*st.fn["order_pens"](ends, group, n_groups, reverse), n, group, True, "the path order is not a permutation that keeps the pens together")
    else:                                                                 # one group, no stroke reversed
        group, n_groups = np.zeros(n, np.int32), 1
        order, rev = _checked_order(st.fn["order"](ends), None, n, group, True, "the path order is not a permutation")
    if o.improve_order:
        lap("order")
        order, rev, ist = st.fn["improve"](ends, group, n_groups, np.asarray(order, np.int32), rev, reverse, o.improve_rounds)
        order, rev = _checked_order(order, rev, n, group, reverse, "the improved order is not a permutation that keeps the pens together and the directions allowed")
        info["improve"] = {k: int(ist[k]) for k in IMPROVE_STATS}
        if greedy is not None and info["improve"]["travel_before"] != info["ring_entry"]["travel"]:
            raise RuntimeError("the ring order and the improvement count different pen-up steps for the same sequence")
        lap("improve")
    return order, rev


def travel_steps(off, pts, start=(0, 0)) -> int:
    """the pen-up steps of strokes drawn as they stand, from `start`: max(|dx|, |dy|) per travel, as the stream compiler counts them"""
    off = np.asarray(off, np.int64); pts = np.asarray(pts, np.int64).reshape(-1, 2)
    if len(off) <= 1:
        return 0
    a, b = pts[off[:-1]], pts[off[1:] - 1]
    return int(np.abs(a - np.concatenate([np.asarray(start, np.int64).reshape(1, 2), b[:-1]])).max(1).sum())


def _stipple(st: StrokeSteps, m: dict, info: dict):
    """the dots of the stippled shapes, (xy, group), in the order the rule states; info["stipple"]"""
    sp = st.stipple
    xy, grp, sst = st.fn["stipple"](sp.ring_sub, sp.ring_group, m, sp.clamp, sp.lattice, sp.inset, sp.rect, sp.flags)
    xy = np.asarray(xy, np.int32).reshape(-1, 2); grp = np.asarray(grp, np.int64).reshape(-1)
    d = {k: int(sst[k]) for k in STIPPLE_STATS}
    (p, q, s), (x0, y0, x1, y1) = sp.lattice, sp.rect
    x, y = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    if len(grp) != len(xy) or d["dots"] != len(xy) or d["candidates"] != d["near"] + d["outside"] + d["hidden"] + d["dots"] or (np.diff(grp) < 0).any() or \
            (d["hidden"] and not sp.flags & STIPPLE_OCCLUDE) or (len(grp) and not np.isin(grp, sp.ring_group).all()):
        raise RuntimeError("the stipple's counts do not add up")
    if (y % q).any() or ((x - np.where((y // q) & 1, s, 0)) % p).any() or ((x < x0) | (x > x1) | (y < y0) | (y > y1)).any():
        raise RuntimeError("the stipple returned a dot off the lattice or outside the rectangle")
    info["stipple"] = dict(d, pitch=p, row=q, shift=s)
    return xy, grp


def _seam(st: StrokeSteps, off, pts, order, rev, info: dict, is_tap=None):
    """the strokes gathered in drawing order, every closed one started at the vertex the pass chose; info["seam"].  is_tap[k]: stroke k is a dot, which the
    pass is sent as the open two-point stroke P, P (its seam is 0)"""
    n = len(off) - 1
    s_off, s_pts = off, pts
    if is_tap is not None and is_tap.any():
        twice = np.ones(len(pts), np.int64); twice[off[:-1][is_tap]] = 2
        s_off = np.concatenate([[0], np.cumsum(np.diff(off) + is_tap)]).astype(np.int64); s_pts = np.repeat(pts, twice, axis=0)
    seam, sst = st.fn["seam"](s_off, s_pts, None if order is None else np.asarray(order, np.int32), None if rev is None else np.asarray(rev, bool))
    seam = np.asarray(seam, np.int64).reshape(-1)
    d = {k: int(sst[k]) for k in SEAM_STATS}
    seq = np.arange(n) if order is None else np.asarray(order, np.int64)
    lens = np.diff(off)[seq]
    closed = (lens >= 4) & (pts[off[:-1][seq]] == pts[off[1:][seq] - 1]).all(1)
    if len(seam) != n or (seam < 0).any() or (seam[~closed] != 0).any() or (seam[closed] >= lens[closed] - 1).any():
        raise RuntimeError("the seams do not name a ring vertex of every closed stroke and 0 for every open one")
    before = gather_paths(off, pts, seq, rev)
    goff, gpts = gather_paths(off, pts, seq, rev, seam)
    if d["closed"] != int(closed.sum()) or d["moved"] != int((seam != 0).sum()) or d["travel_before"] != travel_steps(*before) or d["travel_after"] != travel_steps(goff, gpts) or \
            d["travel_after"] > d["travel_before"] or draw_steps(goff, gpts) != draw_steps(*before):
        raise RuntimeError("the seam pass's counts do not add up")
    if "improve" in info and d["travel_before"] != info["improve"]["travel_after"]:
        raise RuntimeError("the seam pass and the improvement count different pen-up steps for the same sequence")
    if "ring_entry" in info and "improve" not in info and d["travel_before"] != info["ring_entry"]["travel"]:
        raise RuntimeError("the seam pass and the ring order count different pen-up steps for the same sequence")
    info["seam"] = d
    return goff, gpts


def _plan(o: GcodeOptions, sc: ST.StreamConfig, off, pts, path_pen, is_tap=None) -> ST.Plan:
    """every move of the plot; path_pen: the pen of every stroke in drawing order, or None for --color-index throughout; is_tap: the strokes that are dots
    (None: none is)"""
    if not (0 <= int(o.color_index) <= 7):
        raise ValueError("color index 0..7")
    div0 = min(max(int(sc.div_start), 0), 63)                             # set_speed(div_start): written here, and remembered (layout: initial_div)
    if path_pen is not None:
        return plan_pens(off, pts, path_pen, [ST.PEN_UP, 0x40 | div0], sc, is_tap)
    return ST.plan_ops(off, pts, np.zeros(len(off) - 1, bool) if is_tap is None else is_tap, (0, 0), [ST.PEN_UP, 0x40 | div0, 0x08 | int(o.color_index)], False, sc)


def stroke_stream(text_or_paths, opts: Optional[GcodeOptions], device, steps: StrokeSteps, timings: Optional[dict] = None, pens: Optional[np.ndarray] = None,
                  convert: Optional[Callable] = None, force: bool = False) -> Tuple[bytes, dict]:
    """build_stream_from_gcode with the steps as one record: parse, the passes of PASSES that the options and the records of `steps` switch on, plan,
    compile.  --dash-mm gives every path the one pattern unless the door brings a Dash record of its own.  convert, force: resolve_steps'"""
    import time
    o = apply_speed_scale(GcodeOptions(**{f.name: getattr(opts, f.name) for f in fields(GcodeOptions)}) if opts is not None else GcodeOptions())
    W, H = target_size(o)
    sc = stream_config(o)
    rect, tol4 = stroke_options(o)
    own_dash = dash_option(o)
    arc_tol = arc_tolerance(o)
    tm = timings if timings is not None else {}
    t0 = time.perf_counter()

    def lap(name):
        nonlocal t0
        t1 = time.perf_counter(); tm[name] = tm.get(name, 0.0) + (t1 - t0); t0 = t1

    table: Optional[ArcTable] = None
    if isinstance(text_or_paths, (str, bytes, bytearray)):
        tools: Optional[List[int]] = [] if o.tool_pens and pens is None else None
        if arc_tol is not None:
            table, pen_moves = parse_gcode_arcs(text_or_paths, tools)
            if not (table.kind >= ARC_CW).any():                          # no arc: the old parser's paths and the old route, byte for byte
                table = None; tools = None if tools is None else []
        if table is None:
            off_mm, pts_mm, pen_moves = parse_gcode(text_or_paths, tools)
        else:
            off_mm, pts_mm = table.sub_off, None                          # one path per subpath; the points come from the flattening
        if tools is not None:
            pens = np.asarray(tools, np.int64)
    else:
        off_mm, pts_mm = text_or_paths
        off_mm = np.asarray(off_mm, np.int64); pts_mm = np.asarray(pts_mm, np.float64).reshape(-1, 2)
        pen_moves = int((np.diff(off_mm) - 1).clip(0).sum())
    lap("parse")
    info = {"paths_mm": len(off_mm) - 1, "pen_down_moves": pen_moves, "paths": 0, "steps": 0, "target": (W, H)}
    pen_sequence(o.pen_order)
    grouped = pens is not None or bool(o.allow_reverse)                   # the new order; without either, everything below is as it was
    if pens is not None:
        pens = np.asarray(pens, np.int64).reshape(-1)
        if len(pens) != len(off_mm) - 1 or (pens < -1).any() or (pens >= MAX_PENS).any():
            raise ValueError(f"pens: one per path ({len(off_mm) - 1}), each -1 or 0..{MAX_PENS - 1}")
    if len(off_mm) <= 1:
        return EMPTY_STREAM, dict(info, bytes=len(EMPTY_STREAM))
    if not (1 <= W <= MAX_TARGET_STEPS and 1 <= H <= MAX_TARGET_STEPS):
        raise ValueError(f"target size {W} x {H} steps: each side must be in 1..2^30 (step coordinates are int32 on the device)")
    if own_dash is not None and steps.dash is None:                       # --dash-mm: every path gets the pattern
        steps = replace(steps, dash=Dash(np.zeros(len(off_mm) - 1, np.int32), np.full(len(off_mm) - 1, own_dash[1], np.int64), [0, len(own_dash[0])], own_dash[0]))
    need = steps_needed(steps, o, grouped, table is not None)
    st, device = resolve_steps(steps, o, grouped, device, convert, force, table is not None)
    m = dict(scale_x=o.scale_x, scale_y=o.scale_y, offset_x_mm=o.offset_x_mm, offset_y_mm=o.offset_y_mm, steps_per_mm=o.steps_per_mm, W=W, H=H, invert_y=int(bool(o.invert_y)))
    n_groups = MAX_PENS if pens is not None else 1

    def finish(off, pts, pen, group):
        """behind the stroke passes: [the dots], the order, [the seams], the plan, the bytes"""
        is_tap = None
        if st.stipple is not None:
            lap("order")
            xy, dot_group = _stipple(st, m, info)
            info["taps"] = len(xy)
            if len(xy):                                                   # one-point ops behind the strokes, in the order the rule states
                is_tap = np.concatenate([np.zeros(len(off) - 1, bool), np.ones(len(xy), bool)])
                off = np.concatenate([off, off[-1] + 1 + np.arange(len(xy), dtype=np.int64)]); pts = np.concatenate([pts, xy])
                if grouped:
                    dot_pen = np.full(len(xy), -1, np.int64) if pens is None or st.stipple.pen_of is None else np.asarray(st.stipple.pen_of(dot_group), np.int64).reshape(-1)
                    if len(dot_pen) != len(xy) or (dot_pen < -1).any() or (dot_pen >= MAX_PENS).any():
                        raise RuntimeError("the pens of the dots: one per dot, each -1 or a pen")
                    dot_pen = np.where(dot_pen < 0, int(o.color_index), dot_pen)
                    if pens is not None:
                        info["pens"]["paths"] = (np.asarray(info["pens"]["paths"]) + np.bincount(dot_pen, minlength=MAX_PENS)).tolist()
                    pen = np.concatenate([pen, dot_pen])
                    group = np.concatenate([group, (np.argsort(np.asarray(pen_sequence(o.pen_order)))[dot_pen] if pens is not None else np.zeros(len(xy))).astype(np.int32)])
            lap("stipple")
        if len(off) <= 1:                                                 # neither a stroke nor a dot
            return EMPTY_STREAM, dict(info, bytes=len(EMPTY_STREAM))
        greedy = None
        if "ring_entry" in need:                                          # in the greedy order's place; everything behind sees a ring where it is entered
            pts, greedy = _ring_entry(st, o, off, pts, group, n_groups, info)
        order, rev = _order(st, o, off, pts, group, n_groups, info, lap, greedy)
        if "seam" in need:
            lap("order")
            off, pts = _seam(st, off, pts, order, rev, info, is_tap)
            lap("seam")
        elif order is not None:
            off, pts = gather_paths(off, pts, order, rev)
        if is_tap is not None and order is not None:
            is_tap = is_tap[order]
        if grouped:
            (info["pens"] if pens is not None else info)["reversed"] = int(rev.sum())
        lap("order")
        P = _plan(o, sc, off, pts, pen[order] if pens is not None else None, is_tap)
        lap("plan")
        data, table, coff = ST.compile_plan(P, sc, device, st.fn.get("codes"), st.fn.get("pack"), initial_div=int(sc.div_start), lap=lap)
        info.update(steps=int(coff[-1]), bytes=len(data), pieces=len(table.pos), moves=len(P.moves))
        return data, info

    def nothing_left():
        """no stroke is left: the empty stream, unless the dots are still to come"""
        if st.stipple is None:
            return EMPTY_STREAM, dict(info, bytes=len(EMPTY_STREAM))
        if pens is not None and "pens" not in info:
            info["pens"] = {"paths": [0] * MAX_PENS, "unmatched": 0, "reversed": 0}
        return finish(np.zeros(1, np.int64), np.zeros((0, 2), np.int32), *((np.zeros(0, np.int64), np.zeros(0, np.int32)) if grouped else (None, None)))

    n_resident = None
    if table is not None:
        off_f, pts_mm, ast = st.fn["flatten"](table, arc_tol)
        info["arcs"] = dict({"tolerance_mm": arc_tol}, **{k: int(ast[k]) for k in ARC_STATS})
        if pts_mm is None:
            n_resident, off_mm = len(off_mm) - 1, None
        else:
            off_mm = np.asarray(off_f, np.int64); pts_mm = np.asarray(pts_mm, np.float64).reshape(-1, 2)
            if len(off_mm) != len(table.sub_off) or (len(off_mm) and int(off_mm[-1]) != len(pts_mm)):
                raise RuntimeError("the flattening did not return one polyline per path")
        lap("flatten")
    off, pts = _convert(st, off_mm, pts_mm, m, rect, info, n_resident)
    lap("to_steps")
    info["paths"] = n = len(off) - 1
    if n == 0:
        return nothing_left()
    pen, group = _stroke_pens(st, o, pens, n, info) if grouped else (None, None)
    # The list-rewriting passes behind the conversion, as (steps, off, pts, pen, group) -> the same.  A pass that may not leave the list empty has raised
    # by then, so one exit serves all; lap("order") in front of each: the sources and the pens belong to the order's lap
    rewrite = {"dash": lambda st, *s: _dash(st, *s, info), "hatch_link": lambda st, *s: _hatch_link(st, *s, m, info),
               "occlude": lambda st, *s: (st, *_occlude(st, *s, m, info)), "dedup": lambda st, *s: (st, *_dedup(st, *s, n_groups, info)),
               "merge": lambda st, *s: (st, *_merge(st, o, *s, n_groups, info)), "simplify": lambda st, off, pts, *s: (st, *_simplify(st, off, pts, tol4, info), *s)}
    for p in PASSES:
        if p.name in rewrite and p.name in need:
            lap("order")
            st, off, pts, pen, group = rewrite[p.name](st, off, pts, pen, group)
            lap(p.timing)
            if len(off) <= 1:                                             # every stroke lies in a gap or under a shape
                return nothing_left()
    return finish(off, pts, pen, group)


IMPROVE_STATS = ("travel_before", "travel_after", "rounds", "converged_groups", "skipped_groups")
CLIP_STATS = ("segments", "inside", "cut", "outside", "paths_out", "points_out")
DEDUP_STATS = ("segments", "whole", "cut", "covered", "pieces", "paths_out", "points_out", "draw_steps_in", "draw_steps_out")      # include/orip.h: orip_gcode_dedup
OCCLUDE_STATS = ("segments", "whole", "cut", "hidden", "pieces", "collapsed", "paths_out", "points_out", "draw_steps_in", "draw_steps_out")      # include/orip.h: orip_gcode_occlude
DASH_STATS = ("paths_in", "dashed", "dashes", "collapsed", "paths_out", "points_out", "length_in", "length_on")      # include/orip.h: orip_gcode_dash
HATCH_LINK_STATS = ("lines", "in_reach", "eligible", "links", "coincident", "paths_out", "points_out", "link_steps")      # include/orip.h: orip_gcode_hatch_link
HATCH_LINK_REACH_MAX = 1 << 20                # include/orip.h: ORIP_HATCH_LINK_REACH_MAX
STIPPLE_STATS = ("groups", "rows", "candidates", "near", "outside", "hidden", "dots")      # include/orip.h: orip_gcode_stipple
STIPPLE_SERPENTINE, STIPPLE_OCCLUDE, STIPPLE_MAX = 1, 2, 1 << 20      # include/orip.h: ORIP_STIPPLE_SERPENTINE, ORIP_STIPPLE_OCCLUDE; pitch, row and inset at most
SEAM_STATS = ("closed", "moved", "travel_before", "travel_after")      # include/orip.h: orip_gcode_seam
RING_ENTRY_STATS = ("closed", "moved", "candidates", "travel")         # include/orip.h: orip_gcode_order_rings
DASH_UNIT, DASH_MAX_ENTRIES = 256, 64         # include/orip.h: ORIP_DASH_UNIT (dash lengths are in 1/256 step), ORIP_DASH_MAX_ENTRIES
SIMPLIFY_TOL4_MAX = (1 << 17) - 1             # include/orip.h: ORIP_SIMPLIFY_TOL4_MAX


def clip_rect(o) -> Optional[Tuple[int, int, int, int]]:
    """None without --clip, else the clip rectangle (x0, y0, x1, y1) in steps: the sheet of target_size(o) less --clip-margin-mm on every side.  The margin
    belongs to --clip, is not negative and leaves a point at least."""
    if not o.clip:
        if o.clip_margin_mm is not None:
            raise ValueError("--clip-margin-mm needs --clip")
        return None
    W, H = target_size(o)
    margin = 0.0 if o.clip_margin_mm is None else float(o.clip_margin_mm)
    if not (margin >= 0.0) or margin == float("inf"):
        raise ValueError("--clip-margin-mm must be a number and not negative")
    m = margin * float(o.steps_per_mm)
    m = int(round(m)) if m < float(1 << 31) else 1 << 31
    if 2 * m > min(W, H) - 1:
        raise ValueError(f"--clip-margin-mm {margin:g} is {m} steps: nothing is left of a sheet of {W} x {H} steps")
    return m, m, W - 1 - m, H - 1 - m


def simplify_tol4(o) -> Optional[int]:
    """None without --simplify-mm, else the tolerance in quarter steps, round(4 mm steps_per_mm): 0 .. 2^17 - 1"""
    if o.simplify_mm is None:
        return None
    mm = float(o.simplify_mm)
    if not (mm >= 0.0) or mm == float("inf"):
        raise ValueError("--simplify-mm must be a number and not negative")
    q = 4.0 * mm * float(o.steps_per_mm)
    if not (q < float(1 << 31)):
        raise ValueError(f"--simplify-mm {mm:g} at {o.steps_per_mm:g} steps per mm is too wide")
    t = int(round(q))
    if t > SIMPLIFY_TOL4_MAX:
        raise ValueError(f"--simplify-mm {mm:g} is {t / 4:g} steps: at most {SIMPLIFY_TOL4_MAX / 4:g}")
    return t


def dash_entries(lengths: Sequence[float], scale: float) -> Optional[List[int]]:
    """a dash array as the entries of a pattern in 1/256 step, int(round(length scale)) each, an odd count doubled as SVG does; None when an entry would be
    under one step or over 2^40, or when there are none or more than 64: nothing the pass can take"""
    ent = [int(round(float(v) * scale)) for v in lengths]
    ent = ent * 2 if len(ent) % 2 else ent
    if not ent or len(ent) > DASH_MAX_ENTRIES or any(not (DASH_UNIT <= e <= (1 << 40)) for e in ent):
        return None
    return ent


def dash_option(o) -> Optional[Tuple[List[int], int]]:
    """None without --dash-mm, else (the pattern's entries in 1/256 step, the phase): 1 .. 64 lengths in mm, each at least a step; --dash-offset-mm, of any
    sign, reduced mod the pattern's length in Python integers"""
    if o.dash_mm is None:
        if o.dash_offset_mm is not None:
            raise ValueError("--dash-offset-mm needs --dash-mm")
        return None
    scale = float(o.steps_per_mm) * DASH_UNIT
    try:
        mm = [float(tok) for tok in str(o.dash_mm).split(",")]
    except ValueError:
        raise ValueError(f"--dash-mm {o.dash_mm!r}: comma-separated lengths in mm")
    if not (1 <= len(mm) <= DASH_MAX_ENTRIES):
        raise ValueError(f"--dash-mm: {len(mm)} lengths, 1..{DASH_MAX_ENTRIES} are taken")
    for v in mm:
        if not (v >= 0.0) or v == float("inf"):
            raise ValueError(f"--dash-mm {v:g}: a length must be a number and not negative")
        if not (DASH_UNIT <= int(round(v * scale)) <= (1 << 40)):
            raise ValueError(f"--dash-mm {v:g} at {float(o.steps_per_mm):g} steps per mm is {int(round(v * scale)) / DASH_UNIT:g} steps: at least 1, at most 2^32")
    ent = dash_entries(mm, scale)
    if ent is None:
        raise ValueError(f"--dash-mm: {2 * len(mm)} entries once the odd count is doubled, at most {DASH_MAX_ENTRIES}")
    x = 0.0 if o.dash_offset_mm is None else float(o.dash_offset_mm)
    if x != x or x in (float("inf"), float("-inf")):
        raise ValueError("--dash-offset-mm must be a number")
    return ent, int(round(x * scale)) % sum(ent)


def stroke_options(o) -> Tuple[Optional[Tuple[int, int, int, int]], Optional[int]]:
    """the options of the stroke passes, checked together -> (clip rectangle or None, tol4 or None); --improve-order starts from the greedy order, --improve-rounds belongs to it"""
    if o.improve_order and o.no_reorder:
        raise ValueError("--improve-order with --no-reorder: file order was asked for")
    if o.improve_rounds is not None and not o.improve_order:
        raise ValueError("--improve-rounds needs --improve-order")
    if o.improve_rounds is not None and int(o.improve_rounds) < 0:
        raise ValueError("--improve-rounds must not be negative")
    if o.ring_entry and o.no_reorder:
        raise ValueError("--ring-entry with --no-reorder: file order was asked for (--loop-start chooses the seams of a given order)")
    return clip_rect(o), simplify_tol4(o)


def improve_line(tag: str, st: dict) -> str:
    saved = st["travel_before"] - st["travel_after"]
    return (f"[{tag}] improve: pen-up steps {st['travel_before']} -> {st['travel_after']} ({saved} saved), {st['rounds']} rounds, "
            f"{st['converged_groups']} groups converged, {st['skipped_groups']} skipped")


def ring_entry_line(tag: str, st: dict) -> str:
    return (f"[{tag}] ring entry: {st['closed']} closed strokes, {st['moved']} entered away from their first vertex, {st['candidates']} candidates, "
            f"pen-up steps {st['travel']} behind the greedy order")


def seam_line(tag: str, st: dict) -> str:
    saved = st["travel_before"] - st["travel_after"]
    return f"[{tag}] loop start: {st['closed']} closed strokes, {st['moved']} start elsewhere, pen-up steps {st['travel_before']} -> {st['travel_after']} ({saved} saved)"


# ------------------------------------------------------------------ command line (:436-638)
def build_argparser() -> argparse.ArgumentParser:
    d = GcodeOptions()
    ap = argparse.ArgumentParser(description="Convert G-code to an OmniRevolve plotter stream (A4 defaults); ordering and packing run on the GPU.")
    ap.add_argument("input", help="input G-code file")
    ap.add_argument("-o", "--output", default=d.output, help="output stream file")
    ap.add_argument("--target-width-steps", type=int, default=None, help="canvas width in steps (default: A4 width x steps per mm; needs the height too)")
    ap.add_argument("--target-height-steps", type=int, default=None, help="canvas height in steps (default: A4 height x steps per mm; needs the width too)")
    ap.add_argument("--steps-per-mm", type=float, default=d.steps_per_mm)
    ap.add_argument("--invert-y", type=int, default=d.invert_y, help="1: flip Y inside the canvas")
    ap.add_argument("--offset-x-mm", type=float, default=d.offset_x_mm)
    ap.add_argument("--offset-y-mm", type=float, default=d.offset_y_mm)
    ap.add_argument("--scale-x", type=float, default=d.scale_x)
    ap.add_argument("--scale-y", type=float, default=d.scale_y)
    ap.add_argument("--color-index", type=int, default=d.color_index, help="pen 0..7")
    ap.add_argument("--div-start", type=int, default=d.div_start)
    ap.add_argument("--div-fast", type=int, default=d.div_fast)
    ap.add_argument("--profile", choices=["triangle", "scurve"], default=d.profile)
    ap.add_argument("--corner-deg", type=float, default=d.corner_deg)
    ap.add_argument("--corner-div", type=int, default=d.corner_div)
    ap.add_argument("--corner-window-steps", type=int, default=d.corner_window_steps)
    ap.add_argument("--travel-div-fast", type=int, default=d.travel_div_fast)
    ap.add_argument("--travel-start-div", type=int, default=d.travel_start_div)
    ap.add_argument("--travel-window-steps", type=int, default=d.travel_window_steps)
    ap.add_argument("--travel-quant-step", type=int, default=d.travel_quant_step)
    ap.add_argument("--short-len-steps", type=int, default=d.short_len_steps)
    ap.add_argument("--short-div", type=int, default=d.short_div)
    ap.add_argument("--speed-scale", type=float, default=d.speed_scale, help="> 1 faster (smaller dividers), < 1 slower")
    add_stroke_args(ap, STROKE_ARGS[:2])
    ap.add_argument("--tool-pens", action="store_true", help="a path is drawn with the pen its T word names (T0..T7; before any T: --color-index), pen after pen")
    add_stroke_args(ap, STROKE_ARGS[2:])
    ap.add_argument("--loop-start", action="store_true", help="start and end every closed stroke at the vertex that makes the pen-up travel of the whole plot least, "
                                                              "all of them chosen together, after the order (and --improve-order); allowed with --no-reorder")
    ap.add_argument("--dash-mm", default=None, help="draw every path dashed: 1..64 comma-separated lengths in mm, dash and gap in turn (an odd count is repeated, as "
                                                    "in SVG); each at least one step; the pattern starts anew with every path")
    ap.add_argument("--dash-offset-mm", type=float, default=None, help="where in the pattern a path starts (any sign; default 0); needs --dash-mm")
    ap.add_argument("--ring-entry", action="store_true", help="let the greedy order enter a closed stroke at its nearest vertex instead of the one the file lists first "
                                                              "(every ring vertex is a candidate; usually less pen-up travel, nothing promises it); not with --no-reorder")
    ap.add_argument("--arcs", action="store_true", help="draw G2 / G3 as the arcs they state (I / J or R, G90.1 / G91.1, modal), flattened on the GPU with every point on "
                                                        "the circle; without it they are drawn as their chords, as the reference draws them")
    ap.add_argument("--arc-tolerance-mm", type=float, default=None, help="how far a chord may leave its arc, in the file's mm before --scale-x / --scale-y "
                                                                         "(default: half a step on paper); needs --arcs")
    return ap


STROKE_ARGS = ("--no-reorder", "--allow-reverse", "--pen-order", "--merge-paths", "--improve-order", "--improve-rounds", "--clip", "--clip-margin-mm", "--simplify-mm", "--dedup")


def add_stroke_args(ap: argparse.ArgumentParser, names: Sequence[str] = STROKE_ARGS, suffix: str = "") -> None:
    """the options of the stroke passes, those of `names` in that order; `suffix` ends the help of the four that change what is drawn but not the G-code file"""
    flag, number = dict(action="store_true"), dict(default=None)
    table = {
        "--no-reorder": (flag, "keep the paths in file order"),
        "--allow-reverse": (flag, "let the order draw a stroke backwards when its far end is nearer"),
        "--pen-order": (number, "pens in drawing order, comma-separated (default: ascending); pens without paths are skipped"),
        "--merge-paths": (flag, "draw strokes of one pen that meet end to end on the step grid as one stroke (no tolerance; where three or more ends meet, none are joined)" + suffix),
        "--improve-order": (flag, "after the greedy order, lower the pen-up travel by 2-opt (with --allow-reverse) and or-opt moves, one per round, pen by pen" + suffix),
        "--improve-rounds": (dict(number, type=int), "rounds per pen at most (default: 2 m + 64 for m strokes); needs --improve-order"),
        "--clip": (flag, "cut the strokes at the edge of the sheet and lift the pen outside it, instead of clamping every point onto the edge" + suffix),
        "--clip-margin-mm": (dict(number, type=float), "cut this far inside the edge of the sheet (default: 0); needs --clip"),
        "--simplify-mm": (dict(number, type=float), "drop the vertices that lie within this distance of the stroke (Ramer-Douglas-Peucker on the step grid; "
                                                    "0: only vertices on the straight line between their neighbours)"),
        "--dedup": (flag, "draw collinear segments of one pen that lie over each other on the step grid once: the first drawn copy stays (no tolerance)" + suffix),
    }
    for name in names:
        ap.add_argument(name, help=table[name][1], **table[name][0])


def report_lines(tag: str, info: dict, unmatched: bool = False):
    """the lines the tools print about the stroke passes that ran; `unmatched`: the pens line also counts the paths without a stroke colour"""
    if "arcs" in info:
        a = info["arcs"]
        yield f"[{tag}] arcs: {a['arcs']} arcs drawn in {a['pieces']} pieces within {a['tolerance_mm']:g} mm, {a['full_circles']} full circles"
    if "clip" in info:
        c = info["clip"]; x0, y0, x1, y1 = c["rect"]
        yield (f"[{tag}] clip: {c['segments']} segments: {c['inside']} inside, {c['cut']} cut, {c['outside']} outside [{x0}, {x1}] x [{y0}, {y1}] steps -> "
               f"{c['paths_out']} strokes, {c['points_out']} points")
    if "pens" in info:
        yield (f"[{tag}] pens: " + ", ".join(f"{p}: {k} paths" for p, k in enumerate(info["pens"]["paths"]) if k) + "; " +
               (f"{info['pens']['unmatched']} without a stroke colour, " if unmatched else "") + f"{info['pens']['reversed']} strokes reversed")
    if "dash" in info and "dashed" not in info["dash"]:
        yield f"[{tag}] dash: no stroke dashed, {info['dash']['ignored']} dash arrays ignored (under a step, over the limits or all zero): their strokes are solid"
    elif "dash" in info:
        d = info["dash"]
        yield (f"[{tag}] dash: {d['dashed']} strokes dashed, {d['length_on'] / DASH_UNIT:.0f} of {d['length_in'] / DASH_UNIT:.0f} steps drawn in {d['dashes']} dashes, "
               f"{d['collapsed']} under a step dropped" + (f", {d['ignored']} dash arrays ignored" if d.get("ignored") else "") + f" -> {d['paths_out']} strokes")
    if "hatch_link" in info:
        yield (f"[{tag}] " + "hatch connect: {lines} hatch lines, {links} links of at most {reach} steps ({in_reach} pairs in reach, {eligible} inside their shape) -> "
                              "{paths_out} strokes, {link_steps} pen-down steps added".format(**info["hatch_link"]))
    if "occlude" in info:
        yield (f"[{tag}] " + "occlude: {segments} segments: {whole} whole, {cut} cut, {hidden} hidden -> {paths_out} strokes, "
                              "pen-down steps {draw_steps_in} -> {draw_steps_out}".format(**info["occlude"]))
    if "dedup" in info:
        yield (f"[{tag}] " + "dedup: {segments} segments: {whole} whole, {cut} cut, {covered} covered -> {paths_out} strokes, "
                              "pen-down steps {draw_steps_in} -> {draw_steps_out}".format(**info["dedup"]))
    if "merge" in info:
        yield f"[{tag}] " + "merge: {paths_in} paths -> {paths_out}, {joins} pen lifts saved, {cycles} closed".format(**info["merge"])
    if "simplify" in info:
        st = info["simplify"]
        yield f"[{tag}] simplify: {st['points_in']} points -> {st['points_out']} within {st['tol4'] / 4:g} steps, {st['paths_changed']} strokes changed"
    if "stipple" in info:
        d = info["stipple"]
        yield (f"[{tag}] stipple: {d['dots']} dots in {d['groups']} shapes (pitch {d['pitch']}, rows {d['row']}; {d['near']} near the outline, "
               f"{d['outside']} off the sheet, {d['hidden']} hidden)")
    if "ring_entry" in info:
        yield ring_entry_line(tag, info["ring_entry"])
    if "improve" in info:
        yield improve_line(tag, info["improve"])
    if "seam" in info:
        yield seam_line(tag, info["seam"])


def options_from_args(a: argparse.Namespace) -> GcodeOptions:
    return GcodeOptions(**{f.name: getattr(a, f.name) for f in fields(GcodeOptions)})


def main(argv: Optional[Sequence[str]] = None, **device_steps) -> None:
    a = build_argparser().parse_args(argv)
    opts = options_from_args(a)
    apply_speed_scale(GcodeOptions(speed_scale=opts.speed_scale))        # a bad scale ends the run before the file is read, as in the reference
    stroke_options(opts)
    dash_option(opts)
    tol = arc_tolerance(opts)
    text = Path(a.input).read_bytes()
    data, info = build_stream_from_gcode(text, opts, **device_steps)
    Path(a.output).write_bytes(data)
    print(f"[gcode] {a.input}: {info['paths_mm']} pen-down paths, {info['pen_down_moves']} pen-down moves")
    print(f"[gcode] {info['paths']} paths in step space, {info['steps']} steps, target {info['target'][0]} x {info['target'][1]} steps")
    if tol is not None and "arcs" not in info:
        print(f"[gcode] arcs: no G2 / G3 arc in the file; tolerance {tol:g} mm unused")
    for line in report_lines("gcode", info):
        print(line)
    print(f"stream saved: {a.output} ({len(data)} bytes)")


if __name__ == "__main__":
    main()
