"""SVG -> plotter stream: the third front door of the reference (svg_to_stream/svg2stream.py = svg2gcode.py, then gcode2stream.py, then the previewer), in one
process and with the geometry on the device from the control points to the stream bytes.

The XML and the path data are parsed on the host into a SegmentTable (lines, quadratic and cubic Beziers in user units, one 2 x 3 matrix per transformed
element; arcs, circles, ellipses and rounded corners become cubics HERE, pieces of at most 90 degrees with handles 4/3 tan(theta / 4), so the device sees
polynomials only).  The device flattens the curves (orip_svg_flatten), takes the bounding box (orip_svg_bbox) and fits the drawing onto the page with the
reference's 4-decimal rounding (orip_svg_fit); orip_gcode_to_steps then reads the fitted paths where they lie and the rest is orip/gcode.py.

What is the reference's and what is ours.  svg2gcode.py leaves the geometry to the third-party svg_to_gcode package, which is not available to compare
against: the point set chosen for a curve is ours.  It is held to the curve within --tolerance-mm.  It is not the svg_to_gcode package's subdivision, and
neither are the Y-up convention or the element coverage, because that package is not available to compare against.  From the fitted coordinates onward,
every byte is the reference's: the box over all points (:111-141), the aspect-preserving fit (:320-351), v * s + o printed with :.4f (:144-172), and
gcode2stream.py on that text.  viewBox is not applied to the geometry: the reference's docstring says it does not rely on it, and the fit makes a uniform
viewBox scale irrelevant.  Raw Y is canvas height - y (Y-up G-code, [recalled]: DESIGN 5), the height by the rule of ensure_svg_has_size (:57-102).

The tolerance.  The distance between the curve at parameter t and the emitted chord at the same t is at most tolerance_mm in page mm, with the scale that
was finally applied.  The scale depends on the box and the box on the flattening; tolerance_bound() breaks the circle with a bound that holds before any
curve is cut: every curve's end points are in the final point set, so the final box contains the box of the end points alone and the final automatic scale
is at most the scale of that smaller box.  build_stream_from_svg checks the applied scale against the bound afterwards and flattens again only when the
end points' box says nothing (all of them on one point).

Hatch fill (off unless --hatch-spacing-mm is given).  The reference fills shapes in its demo sheet generator (stream_generators/plotter_demo/
omnirevolve_plotter_demo.py, hatch_fill :220-260): scanlines over a group of polygons in integer steps, crossings paired even-odd, both ends inset, every
other line reversed.  Here a fill group is one SVG element (all subpaths of a path, so holes work), chosen by its fill (parse_svg), and orip_svg_hatch
runs that function's rules on the fitted paths after they are quantised to steps; the hatch lines join the fitted paths as 2-point paths in mm, so the
G-code text, the order and the stream treat them like any other path.  Every fill is even-odd, whatever fill-rule says, because the reference's pairing is
(stated deviation), and the SVG default of a black fill is not taken as a request to hatch: only a fill that is written down is.

Hatch angle (--hatch-angle-deg, only with --hatch-spacing-mm; ours, the reference's hatch_fill knows X and Y).  The angle, counter-clockwise in the frame
of the written G-code, is reduced into (-90, 90] and becomes the integer direction u = (round(4096 cos A), round(4096 sin A)) (hatch_direction_vector);
hatch_params adds it as "u", and _Resident.hatch then calls orip_svg_hatch_angle in the place of orip_svg_hatch: one global family of lines n . p = k D,
exact rational crossings, ends rounded to the nearest step (include/orip.h states the rule).  --hatch-direction then means along the angle, across it, or
both; info["hatch"] gains "collapsed"; everything behind the hatch sees ordinary 2-point paths.  0 degrees is NOT --hatch-direction horizontal.

Pens (off unless --pen-colors is given; ours, the reference's svg2stream.py draws with one pen).  parse_svg records the stroke and the fill of every
subpath's element as written (style property, presentation attribute, enclosing groups).  --pen-colors names the colour of each pen; a subpath is drawn
with the pen whose colour is nearest to its stroke -- squared Euclidean distance over the 8-bit sRGB values, in integers, the lowest pen on ties.  That
metric is this module's choice: the reference defines none, and it is NOT the Lab metric of analyze_colors, which lives on the device.  A subpath
without a stated stroke takes --color-index; a hatch line takes the pen of its element's fill colour, or of its stroke where the fill is no colour.
What is drawn does not change (an element with stroke="none" is still drawn, as before: stated deviation).  The pens travel through the hatch
(orip_svg_hatch_groups_fetch) and the conversion to steps (orip_gcode_steps_source_fetch) into orip/gcode.py, which draws pen after pen.

--clip (off unless given; ours, orip/gcode.py states it): a drawing that --scale or a small page pushes over the edge of the sheet is cut there instead
of being clamped onto the edge.  The fitted paths, hatch lines included, are cut where they lie on the device (orip_gcode_to_steps_clip without pointers);
the pens of the cut strokes still come through the sources, and the G-code file is not changed.

--simplify-mm (off unless given; ours, orip/gcode.py states it): the vertices that lie within the given distance of their stroke are dropped, on the step
grid and on the device (orip_gcode_simplify), after the merge and before the order.  It is forwarded as it is; the G-code file is not changed, and
--tolerance-mm keeps its meaning (how far a chord may lie from its curve; this option then thins the chords that the pen cannot tell apart).

--dedup (off unless given; ours, orip/gcode.py states it): collinear segments of one pen that lie over each other on the step grid -- the shared border of
two regions, the inner edges of a table of <rect>s -- are drawn once, on the device (orip_gcode_dedup), after the pens and before the merge.  Hatch lines
go through it like any path.  It is forwarded as it is; the G-code file is not changed.

--occlude (off unless given; ours, svg2stream.py only; include/orip.h states the rule): filled shapes hide what lies under them.  Which elements occlude is
what --hatch-fill decides (fill_group >= 0: one notion of "filled" in the tool).  The parser records the ordinal of every subpath's element, its place in paint
order: that is a path's LEVEL, a hatch line's level is its fill group, and the rings are the filled subpaths with that number -- so a shape hides neither
its own outline nor its own hatch, and everything painted before it where it lies inside, across pens.  The pass runs on the step polylines, on the device
(orip_svg_occlude: the rings are the resident fitted paths, converted there as the strokes were, clamped unless --clip cuts), after the pens have been worked
out and before the dedup, which then removes what is doubled among what is left; the merge rejoins a closed outline that was cut at its start vertex.
Pens and levels follow through origin.  The G-code file is not changed; the preview is rendered from the stream and shows the result.

--dashes (off unless given; ours, svg2stream.py only; include/orip.h states the rule): a stroke that states a stroke-dasharray is drawn as its dashes.  The
parser records stroke-dasharray and stroke-dashoffset per subpath, resolved as the stroke colour is (style property, else presentation attribute, else the
enclosing groups; a unit is dropped); dash_patterns() scales them to 1/256 steps and says which values leave the stroke solid.  The pass runs on the step
polylines, on the device (orip_gcode_dash), after the pens have been worked out and before the occlusion, so a shape on top cuts dashes as it does on a
screen, and the phase counts from the start of every stroke the conversion leaves.  Hatch lines are never dashed.  A drawing that states no dash array gets
no device call.  Declined: dots for zero-length dashes, stroke-linecap, pathLength, vector-effect.  The G-code file is not changed.

--hatch-connect [--hatch-connect-mm M] (off unless given; ours, svg2stream.py only; include/orip.h states the rule): a hatch is drawn as zigzags.  Every
hatch line is a stroke of its own, so a hatched sheet lifts the pen once per line; with the option consecutive lines of one fill group and one hatch family
are joined by straight links of at most M mm (default: twice --hatch-spacing-mm; reach = int(round(M steps_per_mm)) steps, 1 .. 2^20) that lie wholly inside
the shape, so a link never crosses the outline, a hole or a concave corner.  A line's CLASS is 2 g + f: g its fill group (orip_svg_hatch_groups_fetch), f its
family, read off its direction in mm: 0 iff |d . u| >= |d . n|, u = (1, 0) for the hatch along X / Y and the tool's u under --hatch-angle-deg.  The rings
are the subpaths --hatch-fill marks, numbered by their fill group.  The pass runs on the step polylines, on the device (orip_svg_hatch_link: the rings are
the resident fitted paths, converted there as the strokes were, clamped unless --clip cuts), after the pens and the dashes and before the occlusion, so a
shape on top cuts a zigzag as it does on a screen.  Pens, levels and sources follow a zigzag through its first line.  With --hatch-inset-mm 0 the ends lie on
the outline and nothing links; with --no-serpentine a link is a long diagonal, mostly out of reach: the report line says how many lines linked.  The G-code
file is not changed; the preview is rendered from the stream and shows the result.

--stipple-mm S [--stipple-inset-mm I] [--stipple-pattern square|stagger] (off unless given; ours, svg2stream.py only; include/orip.h states the rule): the
shapes --hatch-fill marks are filled with dots, the plotter's taps, on ONE lattice for the whole drawing: pitch = int(round(S steps_per_mm)) steps, 2 .. 2^20;
square = (pitch, pitch, 0), stagger (the default) = (pitch, max(1, (pitch 3547 + 2048) >> 12), pitch >> 1) as (pitch, row distance, shift of the odd rows);
3547 / 4096 stands for sqrt(3) / 2, a stated deviation from a true hexagonal lattice.  A dot lies strictly inside its shape (even-odd, holes work) and at
least I mm (default 0.675, --hatch-inset-mm's default; rounded as the pitch) from its outline, inside the sheet (the clip rectangle under --clip); under
--occlude the dots a shape painted later covers are left out.  --no-serpentine draws every row left to right.  The dots are placed on the device
(orip_svg_stipple: the rings are orip_svg_hatch_link's) after the simplification and join the strokes as one-point ops immediately before the order; with
--pen-colors a dot takes the pen of its shape's fill colour, else of its stroke (hatch_pens).  Independent of --hatch-spacing-mm: both may be on.  The
G-code file is not changed (G-code has no tap); the preview is rendered from the stream and shows the dots.

The device steps are injectable, as in orip/gcode.py, so that this host logic can be tested without a GPU; the product has no CPU path."""
from __future__ import annotations

import argparse
import math
import re
import xml.etree.ElementTree as ET
from dataclasses import dataclass, fields
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import gcode as GC
from .lib import HATCH_SERPENTINE, HATCH_HORIZONTAL, HATCH_VERTICAL

LINE, QUAD, CUBIC = 1, 2, 3
KAPPA = 4.0 / 3.0 * math.tan(math.pi / 8.0)            # handle length of a 90 degree piece, per unit radius
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
SKIPPED = {"defs", "clipPath", "mask", "symbol", "pattern", "marker"}
GROUPS = {"svg", "g", "a", "switch"}


# ------------------------------------------------------------------ the table
@dataclass
class SegmentTable:
    """Flat arrays.  Segment s: kind[s] (LINE / QUAD / CUBIC), ctrl[s] its control points in user units (the unused ones repeat the last), mat[s] the index of
    its matrix in mats (a, b, c, d, e, f: x' = a x + c y + e, y' = b x + d y + f).  Subpath p = segments sub_off[p] .. sub_off[p + 1] - 1, one pen-down path;
    closed[p]: it ended with Z (the closing line is one of its segments).  fill_group[p]: -1, or the ordinal of the element subpath p belongs to when that
    element is to be hatched (parse_svg; None counts as all -1).  stroke_rgb[p], fill_rgb[p]: the colour of the subpath's element as written, 8-bit sRGB, or
    (-1, -1, -1) where none is stated or what is stated is no colour (None counts as all -1).  element[p]: the ordinal of subpath p's element among the
    elements that drew something, its place in paint order (None: not recorded; --occlude needs it).  dash_array[p], dash_offset[p]: stroke-dasharray and
    stroke-dashoffset of the subpath's element as written, or None where nobody states one (lists of strings; None: not recorded; --dashes reads them)."""
    kind: np.ndarray
    ctrl: np.ndarray
    mat: np.ndarray
    sub_off: np.ndarray
    closed: np.ndarray
    mats: np.ndarray
    canvas_height: float = 100.0
    fill_group: Optional[np.ndarray] = None
    stroke_rgb: Optional[np.ndarray] = None
    fill_rgb: Optional[np.ndarray] = None
    element: Optional[np.ndarray] = None
    dash_array: Optional[list] = None
    dash_offset: Optional[list] = None

    @property
    def n_seg(self) -> int: return len(self.kind)
    @property
    def n_sub(self) -> int: return len(self.sub_off) - 1

    def raw_mats(self) -> np.ndarray:
        """the matrices with raw Y = canvas_height - y folded in: what the device applies"""
        m = np.array(self.mats, np.float64).reshape(-1, 6)
        m[:, 1] = -m[:, 1]; m[:, 3] = -m[:, 3]; m[:, 5] = float(self.canvas_height) - m[:, 5]
        return m


def _mul(A, B):
    """A after B"""
    return (A[0] * B[0] + A[2] * B[1], A[1] * B[0] + A[3] * B[1], A[0] * B[2] + A[2] * B[3], A[1] * B[2] + A[3] * B[3],
            A[0] * B[4] + A[2] * B[5] + A[4], A[1] * B[4] + A[3] * B[5] + A[5])


class _Builder:
    def __init__(self):
        self.kind: List[int] = []; self.ctrl: List[Tuple[float, ...]] = []; self.mat: List[int] = []
        self.sub_off = [0]; self.closed: List[int] = []
        self.fill_group: List[int] = []; self.elements = 0; self.element: List[int] = []
        self.stroke_rgb: List[Tuple[int, int, int]] = []; self.fill_rgb: List[Tuple[int, int, int]] = []
        self.dash_array: List[Optional[str]] = []; self.dash_offset: List[Optional[str]] = []
        self.mats: List[Tuple[float, ...]] = [IDENTITY]
        self.m = 0
        self.cur = self.start = (0.0, 0.0)

    def _seg(self, kind, *p):
        q = list(p) + [p[-1]] * (4 - len(p))
        self.kind.append(kind); self.ctrl.append(tuple(v for xy in q for v in xy)); self.mat.append(self.m)
        self.cur = p[-1]

    def end(self, closed=False):
        if len(self.kind) > self.sub_off[-1]:
            self.sub_off.append(len(self.kind)); self.closed.append(int(closed))

    def move(self, x, y):
        self.end(); self.cur = self.start = (x, y)

    def line(self, x, y): self._seg(LINE, self.cur, (x, y))
    def quad(self, x1, y1, x, y): self._seg(QUAD, self.cur, (x1, y1), (x, y))
    def cubic(self, x1, y1, x2, y2, x, y): self._seg(CUBIC, self.cur, (x1, y1), (x2, y2), (x, y))

    def close(self):
        if self.cur != self.start:
            self.line(*self.start)
        self.end(closed=True); self.cur = self.start

    def corner(self, cx, cy, x, y):
        """a quarter of an ellipse from the current point to (x, y); (cx, cy) is where the two tangents meet"""
        x0, y0 = self.cur
        self.cubic(x0 + KAPPA * (cx - x0), y0 + KAPPA * (cy - y0), x + KAPPA * (cx - x), y + KAPPA * (cy - y), x, y)

    def arc(self, rx, ry, rot, large, sweep, x2, y2):
        """SVG implementation notes F.6: end point to centre form, radii corrected, cut into pieces of at most 90 degrees"""
        x1, y1 = self.cur
        if x1 == x2 and y1 == y2:
            return
        rx, ry = abs(rx), abs(ry)
        if rx == 0.0 or ry == 0.0:
            return self.line(x2, y2)
        phi = math.radians(rot % 360.0)
        cp, sp = math.cos(phi), math.sin(phi)
        dx, dy = (x1 - x2) / 2.0, (y1 - y2) / 2.0
        xp, yp = cp * dx + sp * dy, -sp * dx + cp * dy
        lam = xp * xp / (rx * rx) + yp * yp / (ry * ry)
        if lam > 1.0:
            rx *= math.sqrt(lam); ry *= math.sqrt(lam)
        num = rx * rx * ry * ry - rx * rx * yp * yp - ry * ry * xp * xp
        den = rx * rx * yp * yp + ry * ry * xp * xp
        co = math.sqrt(max(0.0, num / den)) * (-1.0 if bool(large) == bool(sweep) else 1.0)
        cxp, cyp = co * rx * yp / ry, -co * ry * xp / rx
        cx, cy = cp * cxp - sp * cyp + (x1 + x2) / 2.0, sp * cxp + cp * cyp + (y1 + y2) / 2.0
        th1 = math.atan2((yp - cyp) / ry, (xp - cxp) / rx)
        dth = math.atan2((-yp - cyp) / ry, (-xp - cxp) / rx) - th1
        if sweep and dth < 0.0: dth += 2.0 * math.pi
        elif not sweep and dth > 0.0: dth -= 2.0 * math.pi
        n = max(1, int(math.ceil(abs(dth) / (math.pi / 2.0) - 1e-9)))
        d = dth / n
        k = 4.0 / 3.0 * math.tan(d / 4.0)

        def at(t):
            c, s = math.cos(t), math.sin(t)
            return (cx + cp * rx * c - sp * ry * s, cy + sp * rx * c + cp * ry * s), (-cp * rx * s - sp * ry * c, -sp * rx * s + cp * ry * c)
        for i in range(n):
            (_, _), (ax, ay) = at(th1 + i * d)
            (ex, ey), (bx, by) = at(th1 + (i + 1) * d)
            if i == n - 1:
                ex, ey = x2, y2
            x0, y0 = self.cur
            self.cubic(x0 + k * ax, y0 + k * ay, ex - k * bx, ey - k * by, ex, ey)

    def table(self, canvas_height) -> SegmentTable:
        self.end()
        return SegmentTable(np.asarray(self.kind, np.int32), np.asarray(self.ctrl, np.float64).reshape(-1, 4, 2), np.asarray(self.mat, np.int32),
                            np.asarray(self.sub_off, np.int64), np.asarray(self.closed, np.uint8), np.asarray(self.mats, np.float64).reshape(-1, 6), float(canvas_height),
                            np.asarray(self.fill_group, np.int32), np.asarray(self.stroke_rgb, np.int16).reshape(-1, 3), np.asarray(self.fill_rgb, np.int16).reshape(-1, 3),
                            np.asarray(self.element, np.int32), list(self.dash_array), list(self.dash_offset))


# ------------------------------------------------------------------ path data
_NUM = re.compile(r"[+-]?(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?")
_SEP = re.compile(r"[\s,]*")
_ARGS = {"M": 2, "L": 2, "H": 1, "V": 1, "C": 6, "S": 4, "Q": 4, "T": 2, "A": 7, "Z": 0}


class _Stop(Exception):
    pass


def tokenize_path(d: str) -> List[Tuple[str, Tuple[float, ...]]]:
    """(command letter, arguments) of every complete command of a path data string, implicit repetitions spelled out (M's as L, m's as l); numbers
    need no separators (1.5.5, -1-2, 1e-3) and an arc's flags may be glued to what follows (a1 1 0 011 1).  Stops in front of the first thing that
    is not a complete command: what came before it stands."""
    out: List[Tuple[str, Tuple[float, ...]]] = []
    pos, cmd = 0, None

    def skip():
        nonlocal pos
        pos = _SEP.match(d, pos).end()

    def num():
        nonlocal pos
        skip()
        m = _NUM.match(d, pos)
        if not m:
            raise _Stop
        pos = m.end()
        return float(m.group())

    def flag():
        nonlocal pos
        skip()
        if pos < len(d) and d[pos] in "01":
            pos += 1
            return float(d[pos - 1])
        raise _Stop
    try:
        while True:
            skip()
            if pos >= len(d):
                break
            ch = d[pos]
            if ch.isalpha():
                if ch.upper() not in _ARGS or (not out and ch.upper() != "M"):
                    break
                cmd = ch; pos += 1
                if ch.upper() == "Z":
                    out.append((ch, ()))
                    continue
            elif cmd is None or cmd.upper() == "Z":
                break
            elif cmd == "M": cmd = "L"
            elif cmd == "m": cmd = "l"
            if cmd.upper() == "A":
                a = (num(), num(), num(), flag(), flag(), num(), num())
            else:
                a = tuple(num() for _ in range(_ARGS[cmd.upper()]))
            out.append((cmd, a))
            if cmd == "M": cmd = "L"
            elif cmd == "m": cmd = "l"
    except _Stop:
        pass
    return out


def _draw_path(b: _Builder, d: str):
    prev = ""
    c2 = q1 = None                                   # the last cubic's second handle, the last quadratic's handle
    first = True
    b.cur = b.start = (0.0, 0.0)
    for cmd, a in tokenize_path(d):
        up = cmd.upper()
        rel = cmd.islower()
        x0, y0 = b.cur
        ox, oy = (x0, y0) if rel else (0.0, 0.0)
        if up == "M" or (first and up == "L"):
            b.move(a[0] + ox, a[1] + oy)
        elif up == "Z": b.close()
        elif up == "L": b.line(a[0] + ox, a[1] + oy)
        elif up == "H": b.line(a[0] + ox, y0)
        elif up == "V": b.line(x0, a[0] + oy)
        elif up == "C":
            b.cubic(a[0] + ox, a[1] + oy, a[2] + ox, a[3] + oy, a[4] + ox, a[5] + oy); c2 = (a[2] + ox, a[3] + oy)
        elif up == "S":
            h = (2.0 * x0 - c2[0], 2.0 * y0 - c2[1]) if prev in "CS" and prev else (x0, y0)
            b.cubic(h[0], h[1], a[0] + ox, a[1] + oy, a[2] + ox, a[3] + oy); c2 = (a[0] + ox, a[1] + oy)
        elif up == "Q":
            b.quad(a[0] + ox, a[1] + oy, a[2] + ox, a[3] + oy); q1 = (a[0] + ox, a[1] + oy)
        elif up == "T":
            q1 = (2.0 * x0 - q1[0], 2.0 * y0 - q1[1]) if prev in "QT" and prev else (x0, y0)
            b.quad(q1[0], q1[1], a[0] + ox, a[1] + oy)
        elif up == "A": b.arc(a[0], a[1], a[2], a[3] != 0.0, a[4] != 0.0, a[5] + ox, a[6] + oy)
        prev = up; first = False
    b.end()


# ------------------------------------------------------------------ elements
_LEN = re.compile(r"^([+-]?\d*\.?\d+(?:[eE][+-]?\d+)?)([a-zA-Z%]*)$")
_TF = re.compile(r"(matrix|translate|scale|rotate|skewX|skewY)\s*\(([^)]*)\)")


def parse_length(s: Optional[str]) -> Optional[float]:
    """'123', '123px', '210mm' -> the number, the unit dropped; anything else -> None"""
    if s is None:
        return None
    m = _LEN.match(s.strip())
    return float(m.group(1)) if m else None


def parse_transform(s: Optional[str]):
    """the product of a transform list, in document order (the first entry is applied last to a point)"""
    M = IDENTITY
    for name, args in _TF.findall(s or ""):
        v = [float(t) for t in _NUM.findall(args)]
        if name == "matrix" and len(v) == 6: T = tuple(v)
        elif name == "translate" and len(v) in (1, 2): T = (1.0, 0.0, 0.0, 1.0, v[0], v[1] if len(v) == 2 else 0.0)
        elif name == "scale" and len(v) in (1, 2): T = (v[0], 0.0, 0.0, v[1] if len(v) == 2 else v[0], 0.0, 0.0)
        elif name == "rotate" and len(v) in (1, 3):
            c, sn = math.cos(math.radians(v[0])), math.sin(math.radians(v[0]))
            T = (c, sn, -sn, c, 0.0, 0.0)
            if len(v) == 3:
                T = _mul(_mul((1.0, 0.0, 0.0, 1.0, v[1], v[2]), T), (1.0, 0.0, 0.0, 1.0, -v[1], -v[2]))
        elif name == "skewX" and len(v) == 1: T = (1.0, 0.0, math.tan(math.radians(v[0])), 1.0, 0.0, 0.0)
        elif name == "skewY" and len(v) == 1: T = (1.0, math.tan(math.radians(v[0])), 0.0, 1.0, 0.0, 0.0)
        else:
            continue
        M = _mul(M, T)
    return M


def canvas_height(root) -> float:
    """the height svg2gcode.py's ensure_svg_has_size leaves on the root (:57-102): its own when width and height are there, else the rounded viewBox
    height, else the rounded height, else 100.  A height that does not read as a number counts as 100."""
    h = root.get("height")
    if h:                                               # a height that is there is never rewritten, whatever the width
        v = parse_length(h)
        return v if v is not None else 100.0
    vb = root.get("viewBox") or root.get("viewbox")
    vb_h = 100.0
    if vb:
        parts = vb.replace(",", " ").split()
        if len(parts) == 4:
            try:
                float(parts[2]); vb_h = float(parts[3])
            except ValueError:
                vb_h = 100.0
    return float(int(round(vb_h)))


def _f(el, name, default=0.0) -> float:
    v = parse_length(el.get(name))
    return default if v is None else v


def _draw_element(b: _Builder, el, tag: str):
    if tag == "path":
        _draw_path(b, el.get("d") or "")
    elif tag == "line":
        b.move(_f(el, "x1"), _f(el, "y1")); b.line(_f(el, "x2"), _f(el, "y2")); b.end()
    elif tag in ("polyline", "polygon"):
        v = [float(t) for t in _NUM.findall(el.get("points") or "")]
        pts = list(zip(v[0::2], v[1::2]))
        if len(pts) >= 2:
            b.move(*pts[0])
            for p in pts[1:]:
                b.line(*p)
            b.close() if tag == "polygon" else b.end()
    elif tag == "rect":
        x, y, w, h = _f(el, "x"), _f(el, "y"), _f(el, "width"), _f(el, "height")
        rx, ry = parse_length(el.get("rx")), parse_length(el.get("ry"))
        if w <= 0.0 or h <= 0.0:
            return
        rx, ry = (ry if rx is None else rx), (rx if ry is None else ry)
        rx, ry = min(max(rx or 0.0, 0.0), w / 2.0), min(max(ry or 0.0, 0.0), h / 2.0)
        if rx == 0.0 or ry == 0.0:
            b.move(x, y); b.line(x + w, y); b.line(x + w, y + h); b.line(x, y + h); b.close()
            return
        b.move(x + rx, y)
        for (lx, ly), (cx, cy), (ex, ey) in (((x + w - rx, y), (x + w, y), (x + w, y + ry)), ((x + w, y + h - ry), (x + w, y + h), (x + w - rx, y + h)),
                                             ((x + rx, y + h), (x, y + h), (x, y + h - ry)), ((x, y + ry), (x, y), (x + rx, y))):
            if (lx, ly) != b.cur:
                b.line(lx, ly)
            b.corner(cx, cy, ex, ey)
        b.close()
    elif tag in ("circle", "ellipse"):
        cx, cy = _f(el, "cx"), _f(el, "cy")
        rx, ry = (_f(el, "r"), _f(el, "r")) if tag == "circle" else (_f(el, "rx"), _f(el, "ry"))
        if rx <= 0.0 or ry <= 0.0:
            return
        b.move(cx + rx, cy)
        b.corner(cx + rx, cy + ry, cx, cy + ry); b.corner(cx - rx, cy + ry, cx - rx, cy)
        b.corner(cx - rx, cy - ry, cx, cy - ry); b.corner(cx + rx, cy - ry, cx + rx, cy)
        b.close()


_FILL = re.compile(r"(?:^|;)\s*fill\s*:\s*([^;]+)")
HATCH_FILLS = ("stated", "all")


def _fill_of(el, inherited: Optional[str]) -> Optional[str]:
    """the element's fill as written: the style property, else the presentation attribute, else what the enclosing groups say; None: nobody says"""
    m = _FILL.search(el.get("style") or "")
    own = m.group(1) if m else el.get("fill")
    return inherited if own is None else own.strip().lower()


_STROKE = re.compile(r"(?:^|;)\s*stroke\s*:\s*([^;]+)")


def _stroke_of(el, inherited: Optional[str]) -> Optional[str]:
    """the element's stroke as written, resolved as _fill_of resolves the fill"""
    m = _STROKE.search(el.get("style") or "")
    own = m.group(1) if m else el.get("stroke")
    return inherited if own is None else own.strip().lower()


_DASHARRAY = re.compile(r"(?:^|;)\s*stroke-dasharray\s*:\s*([^;]+)")
_DASHOFFSET = re.compile(r"(?:^|;)\s*stroke-dashoffset\s*:\s*([^;]+)")


def _dash_of(el, inherited: Optional[str], prop, attr: str) -> Optional[str]:
    """stroke-dasharray or stroke-dashoffset of the element as written, resolved as _stroke_of resolves the stroke"""
    m = prop.search(el.get("style") or "")
    own = m.group(1) if m else el.get(attr)
    return inherited if own is None else own.strip().lower()


def parse_dasharray(s: Optional[str]) -> Optional[List[float]]:
    """the lengths of a stroke-dasharray, separated by commas or white space, a unit dropped as parse_length drops it; None where SVG draws the stroke solid:
    nothing stated, none, or a list that holds a negative, a percentage or something that is no number (an invalid value)"""
    if s is None or s.strip().lower() in ("", "none"):
        return None
    out = []
    for tok in re.split(r"[\s,]+", s.strip().strip(",")):
        v = None if tok.endswith("%") else parse_length(tok)
        if v is None or not (v >= 0.0) or not math.isfinite(v):
            return None
        out.append(v)
    return out


def dash_patterns(table: SegmentTable, fit_scale, steps_per_mm: float, n_paths: int):
    """--dashes: the drawing's own dash arrays as what orip_gcode_dash takes -> (pattern int32 [n_paths], phase int64 [n_paths], pat_off int32, pat_val int64,
    ignored).  Fitted path p < n_sub is subpath p; the paths behind them are hatch lines and are never dashed.  A length in user units becomes 1/256 steps
    by the scale sqrt(|det|) of the subpath's accumulated matrix x sqrt(|sx sy|) of the applied fit x steps per mm x 256, and every entry is rounded by
    itself (int(round())); an odd list is doubled.  Deviation, stated: under a non-uniform transform SVG dashes in the element's own space, so that a dash
    along the stretched axis is longer than one across it; ours measures along the drawn stroke with the mean scale.  The offset is scaled alike and
    reduced mod the pattern's length.  Identical scaled patterns share a table entry.  A list that sums to zero, that has an entry which rounds to under
    one step (SVG draws a dot or nothing for a zero entry; ours draws the stroke solid: stated) or over 2^40, or more than 64 entries after doubling,
    leaves the stroke solid and is counted in `ignored`."""
    pattern = np.full(int(n_paths), -1, np.int32); phase = np.zeros(int(n_paths), np.int64)
    arrays = table.dash_array if table.dash_array is not None else []
    offsets = table.dash_offset if table.dash_offset is not None else []
    if len(arrays) not in (0, table.n_sub) or len(offsets) not in (0, table.n_sub) or n_paths < table.n_sub * bool(arrays):
        raise ValueError(f"{len(arrays)} dash arrays and {len(offsets)} dash offsets for {table.n_sub} subpaths in {n_paths} paths")
    g = math.sqrt(abs(float(fit_scale[0]) * float(fit_scale[1]))) * float(steps_per_mm) * GC.DASH_UNIT
    known, vals, off, ignored = {}, [], [0], 0
    for p, text in enumerate(arrays):
        lengths = parse_dasharray(text)
        if lengths is None:
            continue
        M = table.mats[int(table.mat[int(table.sub_off[p])])]
        k = math.sqrt(abs(float(M[0]) * float(M[3]) - float(M[1]) * float(M[2]))) * g
        ent = GC.dash_entries(lengths, k) if math.isfinite(k) and sum(lengths) > 0.0 else None
        if ent is None:
            ignored += 1
            continue
        if tuple(ent) not in known:
            known[tuple(ent)] = len(off) - 1; vals += ent; off.append(len(vals))
        pattern[p] = known[tuple(ent)]
        x = parse_length(offsets[p]) if offsets else None
        phase[p] = int(round((x or 0.0) * k)) % sum(ent)
    return pattern, phase, np.asarray(off, np.int32), np.asarray(vals, np.int64), ignored


# the 16 basic CSS colour keywords, and orange
COLOR_KEYWORDS = {"black": (0, 0, 0), "silver": (192, 192, 192), "gray": (128, 128, 128), "white": (255, 255, 255), "maroon": (128, 0, 0), "red": (255, 0, 0),
                  "purple": (128, 0, 128), "fuchsia": (255, 0, 255), "green": (0, 128, 0), "lime": (0, 255, 0), "olive": (128, 128, 0), "yellow": (255, 255, 0),
                  "navy": (0, 0, 128), "blue": (0, 0, 255), "teal": (0, 128, 128), "aqua": (0, 255, 255), "orange": (255, 165, 0)}
NO_COLOR = (-1, -1, -1)
_HEX = re.compile(r"^#([0-9a-f]{3}|[0-9a-f]{6})$")
_RGB = re.compile(r"^rgb\(\s*([+-]?\d*\.?\d+)(%?)\s*,\s*([+-]?\d*\.?\d+)(%?)\s*,\s*([+-]?\d*\.?\d+)(%?)\s*\)$")


def parse_color(s: Optional[str]) -> Tuple[int, int, int]:
    """#rgb, #rrggbb, rgb(r, g, b) with integers or percentages (clamped to 0..255), a keyword of COLOR_KEYWORDS, in any letter case -> 8-bit sRGB;
    none, transparent, currentColor, url(...), unknown words and None -> NO_COLOR"""
    if s is None:
        return NO_COLOR
    t = s.strip().lower()
    m = _HEX.match(t)
    if m:
        h = m.group(1)
        if len(h) == 3:
            h = "".join(ch * 2 for ch in h)
        return int(h[0:2], 16), int(h[2:4], 16), int(h[4:6], 16)
    m = _RGB.match(t)
    if m:
        v = [(m.group(i), m.group(i + 1)) for i in (1, 3, 5)]
        if len({pc for _, pc in v}) != 1 or (v[0][1] == "" and any("." in num for num, _ in v)):
            return NO_COLOR                                  # integers and percentages do not mix, and a plain value is an integer
        return tuple(min(255, max(0, int(round(float(num) * 255.0 / 100.0)) if pc else int(num))) for num, pc in v)
    return COLOR_KEYWORDS.get(t, NO_COLOR)


def parse_pen_colors(spec: str) -> List[Tuple[int, int, int]]:
    """--pen-colors: 1..8 comma-separated colours (#rgb, #rrggbb or a keyword), position = pen; the word rgbk: the previewer's default palette"""
    from .stream_preview import DEFAULT_PALETTE
    if spec.strip().lower() == "rgbk":
        return [tuple(int(v) for v in c) for c in DEFAULT_PALETTE]
    out = [parse_color(tok) for tok in spec.split(",")]
    if not (1 <= len(out) <= GC.MAX_PENS) or any(c == NO_COLOR or "(" in tok for c, tok in zip(out, spec.split(","))):
        raise ValueError(f"--pen-colors: 1..{GC.MAX_PENS} comma-separated colours (#rgb, #rrggbb or a keyword), or rgbk")
    return out


def nearest_pen(rgb, palette) -> np.ndarray:
    """per row of rgb int [n, 3] the palette entry at the smallest squared Euclidean distance over 8-bit sRGB, integers, the lowest index on ties; -1 for
    a row that is NO_COLOR.  Ours: the reference defines no such mapping, and this is not the Lab metric of analyze_colors."""
    c = np.asarray(rgb, np.int64).reshape(-1, 3)
    pal = np.asarray(palette, np.int64).reshape(-1, 3)
    d = ((c[:, None, :] - pal[None, :, :]) ** 2).sum(2)
    return np.where((c < 0).any(1), -1, np.argmin(d, 1)).astype(np.int64)      # argmin: the first minimum


def subpath_pens(table: SegmentTable, palette) -> np.ndarray:
    """the pen of every subpath by its stroke; -1: no stroke stated (the caller's --color-index)"""
    if table.stroke_rgb is None:
        return np.full(table.n_sub, -1, np.int64)
    return nearest_pen(table.stroke_rgb, palette)


def hatch_pens(table: SegmentTable, groups, palette) -> np.ndarray:
    """the pen of every hatch line from its fill group (an element's ordinal): the pen of the element's fill colour, or of its stroke where the fill is
    not a colour (--hatch-fill all); -1 where neither is"""
    groups = np.asarray(groups, np.int64).reshape(-1)
    fg = np.asarray(table.fill_group, np.int64).reshape(-1) if table.fill_group is not None else np.zeros(0, np.int64)
    if len(groups) == 0:
        return np.zeros(0, np.int64)
    if len(fg) == 0 or groups.min() < 0 or groups.max() > fg.max():
        raise RuntimeError("the hatch lines name fill groups the table does not have")
    first = np.full(int(fg.max()) + 1, -1, np.int64)                       # a subpath of every group: all of an element's subpaths share its colours
    sub = np.nonzero(fg >= 0)[0][::-1]
    first[fg[sub]] = sub
    if (first[groups] < 0).any():
        raise RuntimeError("the hatch lines name fill groups the table does not have")
    none = np.full((table.n_sub, 3), -1, np.int64)
    fill = nearest_pen(none if table.fill_rgb is None else table.fill_rgb, palette)
    pen = np.where(fill >= 0, fill, subpath_pens(table, palette))
    return pen[first[groups]]


def _walk(b: _Builder, el, m: int, fill: Optional[str] = None, fill_all: bool = False, stroke: Optional[str] = None, dash: Optional[str] = None,
          dash_at: Optional[str] = None):
    tag = el.tag.rsplit("}", 1)[-1] if isinstance(el.tag, str) else ""
    if not tag or tag in SKIPPED or (el.get("display") or "").strip() == "none":
        return
    fill = _fill_of(el, fill)
    stroke = _stroke_of(el, stroke)
    dash = _dash_of(el, dash, _DASHARRAY, "stroke-dasharray"); dash_at = _dash_of(el, dash_at, _DASHOFFSET, "stroke-dashoffset")
    if el.get("transform"):
        b.mats.append(_mul(b.mats[m], parse_transform(el.get("transform"))))
        m = len(b.mats) - 1
    if tag in GROUPS:
        for ch in el:
            _walk(b, ch, m, fill, fill_all, stroke, dash, dash_at)
    else:
        b.m = m
        _draw_element(b, el, tag)
        b.end()
        new = len(b.closed) - len(b.fill_group)
        if new:                                             # an element that drew something: the next ordinal, whether it is filled or not
            wanted = tag != "line" and (fill_all or (fill is not None and fill not in ("none", "transparent")))
            b.fill_group.extend([b.elements if wanted else -1] * new); b.element.extend([b.elements] * new)
            b.stroke_rgb.extend([parse_color(stroke)] * new); b.fill_rgb.extend([parse_color(fill)] * new)
            b.dash_array.extend([dash] * new); b.dash_offset.extend([dash_at] * new)
            b.elements += 1


def parse_svg(text: Union[str, bytes], hatch_fill: str = "stated") -> SegmentTable:
    """hatch_fill decides table.fill_group: "stated" marks an element whose fill (style property or presentation attribute, its own or inherited from a
    group) is written down and is not none / transparent; "all" marks every element that draws.  A line is never marked."""
    if hatch_fill not in HATCH_FILLS:
        raise ValueError("--hatch-fill must be one of " + ", ".join(HATCH_FILLS))
    root = ET.fromstring(text)
    b = _Builder()
    _walk(b, root, 0, None, hatch_fill == "all")
    return b.table(canvas_height(root))


# ------------------------------------------------------------------ options, fit, tolerance
@dataclass
class SvgOptions:
    """The command lines of svg2gcode.py (:178-259) and svg2stream.py (:34-156): same names, same defaults; tolerance_mm is ours (None: half a step)."""
    output: str = "from_svg.gcode"
    movement_speed: float = 8000.0
    cutting_speed: float = 2000.0
    passes: int = 1
    pass_depth: float = 0.0
    page_width_mm: float = 210.0
    page_height_mm: float = 297.0
    margin_mm: float = 10.0
    scale: Optional[float] = None
    scale_x: Optional[float] = None
    scale_y: Optional[float] = None
    output_stream: Optional[str] = None
    gcode_output: Optional[str] = None
    steps_per_mm: float = 40.0
    target_width_steps: Optional[int] = None
    target_height_steps: Optional[int] = None
    invert_y: int = 0
    color_index: int = 3
    speed_scale: float = 1.0
    no_reorder: bool = False
    no_preview: bool = False
    preview_render_width: int = 1200
    preview_render_height: int = 900
    tolerance_mm: Optional[float] = None
    hatch_spacing_mm: Optional[float] = None            # None: no hatching
    hatch_inset_mm: float = 27.0 / 40.0                 # the reference's 27 steps at 40 steps per mm
    hatch_direction: str = "horizontal"
    no_serpentine: bool = False
    hatch_fill: str = "stated"
    hatch_angle_deg: Optional[float] = None             # None: the reference's hatch along X / Y; else the exact hatch along that angle (orip_svg_hatch_angle)
    hatch_connect: bool = False                         # hatch lines are joined into zigzags by links that stay inside the shape (svg2stream.py only)
    hatch_connect_mm: Optional[float] = None            # the longest link; None: twice hatch_spacing_mm; only with hatch_connect
    stipple_mm: Optional[float] = None                  # filled shapes are filled with dots (taps) this far apart (svg2stream.py only); None: no dots
    stipple_inset_mm: Optional[float] = None            # how far every dot stays inside its shape's outline; None: hatch_inset_mm's default; only with stipple_mm
    stipple_pattern: Optional[str] = None               # square or stagger; None: stagger; only with stipple_mm
    pen_colors: Optional[str] = None                    # None: one pen, --color-index
    pen_order: Optional[str] = None
    allow_reverse: bool = False
    merge_paths: bool = False                           # strokes of one pen that meet end to end on the step grid are drawn as one (orip.gcode)
    improve_order: bool = False                         # 2-opt / or-opt on the order, per pen group (orip.gcode)
    improve_rounds: Optional[int] = None                # rounds per group at most; None: 2 m + 64
    clip: bool = False                                  # strokes are cut at the sheet's edge instead of clamped to it (orip.gcode)
    clip_margin_mm: Optional[float] = None              # the clip rectangle lies this far inside the sheet; None: 0
    simplify_mm: Optional[float] = None                 # vertices within this distance of the stroke are dropped (orip.gcode); None: none are
    dedup: bool = False                                 # collinear segments of one pen that lie over each other are drawn once (orip.gcode)
    loop_start: bool = False                            # closed strokes start at the vertex that makes the pen-up travel least (orip.gcode)
    ring_entry: bool = False                            # the greedy order enters a closed stroke at its nearest ring vertex (orip.gcode)
    occlude: bool = False                               # filled shapes hide what lies under them (svg2stream.py only)
    dashes: bool = False                                # stroke-dasharray is drawn as dashes (svg2stream.py only)


HATCH_DIRECTIONS = {"horizontal": HATCH_HORIZONTAL, "vertical": HATCH_VERTICAL, "cross": HATCH_HORIZONTAL | HATCH_VERTICAL}
HATCH_MAX_STEPS_PER_MM = 5000.0
HATCH_U_SCALE = 4096


def hatch_direction_vector(angle_deg: float) -> Tuple[int, int]:
    """--hatch-angle-deg as the integer direction orip_svg_hatch_angle takes: the angle reduced into (-90, 90], then (round(4096 cos A), round(4096 sin A))"""
    a = float(angle_deg)
    if not math.isfinite(a):
        raise ValueError("--hatch-angle-deg must be finite")
    a = math.fmod(a, 180.0)
    if a > 90.0:
        a -= 180.0
    elif a <= -90.0:
        a += 180.0
    r = math.radians(a)
    return int(round(HATCH_U_SCALE * math.cos(r))), int(round(HATCH_U_SCALE * math.sin(r)))


def hatch_effective_angle(u) -> float:
    """the angle, in degrees, of the direction the hatch really takes"""
    return math.degrees(math.atan2(int(u[1]), int(u[0])))


def hatch_params(o: SvgOptions) -> Optional[dict]:
    """None without --hatch-spacing-mm, else what orip_svg_hatch takes: spacing and inset in steps, the flags, steps per mm.  Above 5000 steps per mm the
    four decimals of the G-code no longer name every step, so the written file and the stream could disagree: refused.  Only with --hatch-angle-deg the
    key "u": the direction orip_svg_hatch_angle takes, which is then the call that hatches."""
    if o.hatch_spacing_mm is None:
        return None
    u = None if o.hatch_angle_deg is None else hatch_direction_vector(o.hatch_angle_deg)
    spm = float(o.steps_per_mm)
    if not (0.0 < spm <= HATCH_MAX_STEPS_PER_MM):
        raise ValueError(f"hatching needs --steps-per-mm in (0, {HATCH_MAX_STEPS_PER_MM:g}]: beyond it four decimals of a mm do not name every step")
    if o.hatch_direction not in HATCH_DIRECTIONS:
        raise ValueError("--hatch-direction must be one of " + ", ".join(HATCH_DIRECTIONS))
    if o.hatch_fill not in HATCH_FILLS:
        raise ValueError("--hatch-fill must be one of " + ", ".join(HATCH_FILLS))
    s, i = float(o.hatch_spacing_mm) * spm, float(o.hatch_inset_mm) * spm
    if not (math.isfinite(s) and math.isfinite(i)) or abs(s) >= 2 ** 31 - 1 or abs(i) >= 2 ** 31 - 1:
        raise ValueError("--hatch-spacing-mm and --hatch-inset-mm must be finite and below 2^31 steps")
    spacing, inset = int(round(s)), int(round(i))
    if spacing < 1:
        raise ValueError(f"--hatch-spacing-mm {o.hatch_spacing_mm} is {spacing} steps at {spm:g} steps per mm: at least 1")
    if inset < 0:
        raise ValueError("--hatch-inset-mm must not be negative")
    prm = {"spacing": spacing, "inset": inset, "flags": HATCH_DIRECTIONS[o.hatch_direction] | (0 if o.no_serpentine else HATCH_SERPENTINE), "steps_per_mm": spm}
    if u is not None:
        prm["u"] = u
    return prm


def hatch_connect_reach(o: SvgOptions) -> Optional[int]:
    """None without --hatch-connect, else the longest link in steps, int(round(M steps_per_mm)) for M = --hatch-connect-mm (default: twice
    --hatch-spacing-mm): 1 .. 2^20.  Both options belong to a hatch, and the length to --hatch-connect."""
    if not o.hatch_connect:
        if o.hatch_connect_mm is not None:
            raise ValueError("--hatch-connect-mm needs --hatch-connect")
        return None
    if o.hatch_spacing_mm is None:
        raise ValueError("--hatch-connect needs --hatch-spacing-mm: there is no hatch to connect")
    mm = 2.0 * float(o.hatch_spacing_mm) if o.hatch_connect_mm is None else float(o.hatch_connect_mm)
    if not (mm > 0.0 and math.isfinite(mm)):
        raise ValueError("--hatch-connect-mm must be a positive number" if o.hatch_connect_mm is not None else "--hatch-connect needs a positive --hatch-spacing-mm")
    r = mm * float(o.steps_per_mm)
    reach = int(round(r)) if math.isfinite(r) and r < float(1 << 31) else 1 << 31
    if not (1 <= reach <= GC.HATCH_LINK_REACH_MAX):
        raise ValueError(f"--hatch-connect-mm {mm:g} is {reach} steps at {float(o.steps_per_mm):g} steps per mm: 1 .. 2^20")
    return reach


STIPPLE_PATTERNS = ("square", "stagger")


def stipple_lattice(pitch: int, pattern: str) -> Tuple[int, int, int]:
    """(pitch, row, shift) of orip_svg_stipple: square = (p, p, 0); stagger = (p, max(1, (p * 3547 + 2048) >> 12), p >> 1), every other row moved by half
    a pitch and the rows 3547 / 4096 of a pitch apart.  That is sqrt(3) / 2 to four digits and then rounded to whole steps: a stated deviation from a true
    hexagonal lattice, whose rows no step grid holds."""
    if pattern not in STIPPLE_PATTERNS:
        raise ValueError("--stipple-pattern must be one of " + ", ".join(STIPPLE_PATTERNS))
    p = int(pitch)
    return (p, p, 0) if pattern == "square" else (p, max(1, (p * 3547 + 2048) >> 12), p >> 1)


def stipple_params(o: SvgOptions) -> Optional[dict]:
    """None without --stipple-mm, else what orip_svg_stipple takes: "lattice" = (pitch, row, shift) with pitch = int(round(S steps_per_mm)) in 2 .. 2^20,
    and "inset" = int(round(I steps_per_mm)) in 0 .. 2^20, I = --stipple-inset-mm (default: --hatch-inset-mm's default).  The inset and the pattern belong
    to --stipple-mm."""
    if o.stipple_mm is None:
        if o.stipple_inset_mm is not None or o.stipple_pattern is not None:
            raise ValueError("--stipple-inset-mm and --stipple-pattern need --stipple-mm")
        return None
    mm, spm = float(o.stipple_mm), float(o.steps_per_mm)
    if not (mm > 0.0 and math.isfinite(mm)):
        raise ValueError("--stipple-mm must be a positive number")
    v = mm * spm
    pitch = int(round(v)) if math.isfinite(v) and v < float(1 << 31) else 1 << 31
    if not (2 <= pitch <= GC.STIPPLE_MAX):
        raise ValueError(f"--stipple-mm {mm:g} is {pitch} steps at {spm:g} steps per mm: 2 .. 2^20")
    im = SvgOptions.hatch_inset_mm if o.stipple_inset_mm is None else float(o.stipple_inset_mm)
    if not (im >= 0.0 and math.isfinite(im)):
        raise ValueError("--stipple-inset-mm must be a number and not negative")
    v = im * spm
    inset = int(round(v)) if math.isfinite(v) and v < float(1 << 31) else 1 << 31
    if inset > GC.STIPPLE_MAX:
        raise ValueError(f"--stipple-inset-mm {im:g} is {inset} steps at {spm:g} steps per mm: at most 2^20")
    return {"lattice": stipple_lattice(pitch, "stagger" if o.stipple_pattern is None else o.stipple_pattern), "inset": inset}


def tolerance_mm(o: SvgOptions) -> float:
    t = 0.5 / float(o.steps_per_mm) if o.tolerance_mm is None else float(o.tolerance_mm)
    if not (t > 0.0 and math.isfinite(t)):
        raise ValueError("--tolerance-mm must be a positive number")
    return t


def _avail(o: SvgOptions) -> Tuple[float, float]:
    return max(1e-6, o.page_width_mm - 2.0 * o.margin_mm), max(1e-6, o.page_height_mm - 2.0 * o.margin_mm)


def _user_scales(o: SvgOptions) -> Tuple[Optional[float], Optional[float]]:
    sx = sy = o.scale
    if o.scale_x is not None: sx = o.scale_x
    if o.scale_y is not None: sy = o.scale_y
    return sx, sy


def fit_transform(bbox, o: SvgOptions) -> Tuple[float, float, float, float]:
    """(sx, sy, offset_x, offset_y) of svg2gcode.py:320-351 in Python floats.  A box of zero width or height: the reference copies its text unfitted;
    ours is not text, so the paths go through the same rounding with s = 1, o = 0 (stated deviation)."""
    min_x, min_y, max_x, max_y = (float(v) for v in bbox)
    width, height = max_x - min_x, max_y - min_y
    if width <= 0 or height <= 0:
        return 1.0, 1.0, 0.0, 0.0
    aw, ah = _avail(o)
    auto = min(aw / width, ah / height)
    ux, uy = _user_scales(o)
    sx = auto if ux is None else ux
    sy = auto if uy is None else uy
    return sx, sy, o.margin_mm - min_x * sx, o.margin_mm - min_y * sy


def tolerance_bound(table: SegmentTable, o: SvgOptions) -> float:
    """An upper bound of the largest scale fit_transform can return for this table, from its end points alone (module docstring).  Along an axis on
    which all end points agree that axis says nothing; if both do, the control hull stands in (a guess, checked after the fact by the caller).  Such
    a drawing may also come out with a box of zero width or height, which is fitted with scale 1."""
    ux, uy = _user_scales(o)
    m = table.raw_mats()[table.mat]
    last = np.take_along_axis(table.ctrl, np.clip(table.kind, 1, 3).reshape(-1, 1, 1).repeat(2, 2).astype(np.int64), 1)[:, 0]

    def raw(p):
        return np.stack([m[:, 0] * p[:, 0] + m[:, 2] * p[:, 1] + m[:, 4], m[:, 1] * p[:, 0] + m[:, 3] * p[:, 1] + m[:, 5]], 1)
    ends = np.concatenate([raw(table.ctrl[:, 0]), raw(last)])
    aw, ah = _avail(o)

    def scales(p):
        w, h = np.ptp(p[:, 0]), np.ptp(p[:, 1])
        return [a / e for a, e in ((aw, w), (ah, h)) if e > 0], w > 0 and h > 0
    cand, full = scales(ends)
    if not cand:
        cand, _ = scales(np.concatenate([raw(table.ctrl[:, j]) for j in range(4)]))
    bound = [abs(u) for u in (ux, uy) if u is not None]
    if len(bound) < 2:
        bound.append(min(cand) if cand else 1.0)
    if not full:
        bound.append(1.0)
    return max(bound) or 1.0


def gcode_options(o: SvgOptions) -> GC.GcodeOptions:
    """what svg2stream.py forwards to gcode2stream.py (:264-290): scale 1, offsets 0, the canvas from the page unless both sizes are given"""
    if o.target_width_steps is not None and o.target_height_steps is not None:
        W, H = int(o.target_width_steps), int(o.target_height_steps)
    else:
        W, H = int(round(o.page_width_mm * o.steps_per_mm)), int(round(o.page_height_mm * o.steps_per_mm))
    return GC.GcodeOptions(steps_per_mm=o.steps_per_mm, invert_y=o.invert_y, color_index=o.color_index, speed_scale=o.speed_scale, scale_x=1.0, scale_y=1.0,
                           offset_x_mm=0.0, offset_y_mm=0.0, target_width_steps=W, target_height_steps=H, no_reorder=bool(o.no_reorder),
                           allow_reverse=bool(o.allow_reverse), pen_order=o.pen_order, merge_paths=bool(o.merge_paths),
                           improve_order=bool(o.improve_order), improve_rounds=o.improve_rounds, clip=bool(o.clip), clip_margin_mm=o.clip_margin_mm,
                           simplify_mm=o.simplify_mm, dedup=bool(o.dedup), loop_start=bool(o.loop_start), ring_entry=bool(o.ring_entry))


def gcode_text(off, pts, passes: int = 1, pens=None) -> str:
    """the fitted paths in a dialect the reference's parser reads: G21, G90, M5; per path G0 to its first point, M3, one G1 per further point, M5.  With
    pens (one per path, 0..7) a line T<pen> stands in front of every path whose pen differs from the one before it; both parsers skip T words, and
    gcode2stream.py --tool-pens honours them."""
    off = np.asarray(off, np.int64); pts = np.asarray(pts, np.float64).reshape(-1, 2)
    xy = ["X%.4f Y%.4f" % (x, y) for x, y in pts.tolist()]
    out = ["G21", "G90", "M5"]
    tools = None if pens is None else np.asarray(pens, np.int64).reshape(-1).tolist()
    if tools is not None and len(tools) != len(off) - 1:
        raise ValueError(f"{len(tools)} pens for {len(off) - 1} paths")
    tool = None
    for _ in range(max(1, int(passes))):
        for p, (a, b) in enumerate(zip(off[:-1].tolist(), off[1:].tolist())):
            if b - a < 1:
                continue
            if tools is not None and tools[p] != tool:
                tool = tools[p]; out.append("T%d" % tool)
            out.append("G0 " + xy[a]); out.append("M3")
            out.extend("G1 " + s for s in xy[a + 1:b])
            out.append("M5")
    return "\n".join(out) + "\n"


class _Resident:
    """the device steps; `paths` is only a count, the points stay where orip_svg_flatten left them"""
    def __init__(self, dev): self.dev = dev
    def flatten(self, table, tol): return {"n": table.n_sub, "total": self.dev.svg_flatten(table, tol)}
    def bbox(self, paths): return self.dev.svg_bbox()
    def fit(self, paths, sx, sy, ox, oy): self.dev.svg_fit(sx, sy, ox, oy); return paths
    def fetch(self, paths, with_points=True): return self.dev.svg_paths(paths["n"], with_points)
    def steps(self, paths, m): return self.dev.gcode_to_steps(None, None, m, n=paths["n"])
    def clip(self, paths, m, rect): return self.dev.gcode_to_steps_clip(None, None, m, rect, n=paths["n"])

    def hatch(self, paths, fill_group, prm):
        if "u" in prm:
            st = self.dev.svg_hatch_angle(fill_group, prm["steps_per_mm"], prm["spacing"], prm["inset"], prm["u"], prm["flags"])
        else:
            st = self.dev.svg_hatch(fill_group, prm["steps_per_mm"], prm["spacing"], prm["inset"], prm["flags"])
        return {"n": paths["n"] + st["segments"], "total": paths["total"] + 2 * st["segments"]}, st

    def hatch_groups(self, paths, segments): return self.dev.svg_hatch_groups(segments)
    def source(self, n): return self.dev.gcode_steps_source(n)


MAX_REFLATTEN = 8


def fit_paths(table: SegmentTable, o: SvgOptions, flatten_fn, bbox_fn, fit_fn, tm: Optional[dict] = None):
    """flatten -> bbox -> fit with the tolerance kept: (paths, {"tol_raw", "scale": (sx, sy, ox, oy), "bbox", "flattens"})"""
    import time
    tm = tm if tm is not None else {}

    def lap(name, t0):
        tm[name] = tm.get(name, 0.0) + (time.perf_counter() - t0)
    tol = tolerance_mm(o)
    tol_raw = tol / tolerance_bound(table, o)
    for k in range(MAX_REFLATTEN):
        t0 = time.perf_counter(); paths = flatten_fn(table, tol_raw); lap("flatten", t0)
        t0 = time.perf_counter(); box = tuple(float(v) for v in bbox_fn(paths)); lap("bbox", t0)
        sx, sy, ox, oy = fit_transform(box, o)
        if max(abs(sx), abs(sy)) * tol_raw <= tol * (1.0 + 1e-12):
            break
        tol_raw = tol / max(abs(sx), abs(sy)) / 2.0           # only where the end points' box said nothing: take the measured scale, with room for the box to shrink
    else:
        raise RuntimeError("the tolerance could not be met: the scale keeps growing as the curves are cut finer")
    t0 = time.perf_counter(); paths = fit_fn(paths, sx, sy, ox, oy); lap("fit", t0)
    return paths, {"tol_raw": tol_raw, "scale": (sx, sy, ox, oy), "bbox": box, "flattens": k + 1}


def path_pens(table: SegmentTable, o: SvgOptions, paths, info: dict, hatch_groups_fn: Optional[Callable]) -> Optional[np.ndarray]:
    """None without --pen-colors, else the pen of every fitted path, hatch lines included (-1: --color-index); info["pen_colors"] = the palette"""
    if o.pen_colors is None:
        return None
    palette = parse_pen_colors(o.pen_colors)
    info["pen_colors"] = palette
    pens = subpath_pens(table, palette)
    seg = int(info["hatch"]["segments"]) if "hatch" in info else 0
    if seg:
        groups = np.asarray(hatch_groups_fn(paths, seg), np.int64).reshape(-1)
        if len(groups) != seg:
            raise RuntimeError(f"{len(groups)} fill groups for {seg} hatch lines")
        pens = np.concatenate([pens, hatch_pens(table, groups, palette)])
    return pens


def occlusion_rings(table: SegmentTable):
    """--occlude: the subpaths that hide, (ring_sub, ring_level) -- those of the elements --hatch-fill marks, the one notion of "filled" in the tool, each
    with its element's ordinal, its place in paint order; ascending as the parser leaves them"""
    if table.element is None or table.fill_group is None:
        raise ValueError("--occlude needs the element ordinals and the fill groups of a parsed SVG")
    fg = np.asarray(table.fill_group, np.int64).reshape(-1); el = np.asarray(table.element, np.int64).reshape(-1)
    if len(fg) != table.n_sub or len(el) != table.n_sub or (el < 0).any() or (np.diff(el) < 0).any() or ((fg >= 0) & (fg != el)).any():
        raise ValueError("the element ordinals must ascend, one per subpath, and a fill group is its element's ordinal")
    sub = np.nonzero(fg >= 0)[0]
    return sub.astype(np.int32), fg[sub].astype(np.int32)


def path_levels(table: SegmentTable, paths, info: dict, hatch_groups_fn: Optional[Callable]) -> np.ndarray:
    """--occlude: the level of every fitted path: a subpath's is its element's ordinal, a hatch line's is its fill group, so a shape hides neither its own
    outline nor its own hatch"""
    level = np.asarray(table.element, np.int64).reshape(-1)
    seg = int(info["hatch"]["segments"]) if "hatch" in info else 0
    if seg:
        groups = np.asarray(hatch_groups_fn(paths, seg), np.int64).reshape(-1)
        if len(groups) != seg or (groups < 0).any():
            raise RuntimeError(f"{len(groups)} fill groups for {seg} hatch lines")
        level = np.concatenate([level, groups])
    return level


def hatch_link_rings(table: SegmentTable):
    """--hatch-connect: the outlines of the hatched shapes, (ring_sub, ring_group) -- the subpaths --hatch-fill marks, as occlusion_rings collects them,
    each with its fill group, the groups ascending (the order inside a group is kept)"""
    if table.fill_group is None:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    fg = np.asarray(table.fill_group, np.int64).reshape(-1)
    if len(fg) != table.n_sub:
        raise ValueError(f"fill_group has {len(fg)} entries for {table.n_sub} subpaths")
    sub = np.nonzero(fg >= 0)[0]
    sub = sub[np.argsort(fg[sub], kind="stable")]
    return sub.astype(np.int32), fg[sub].astype(np.int32)


def hatch_classes(table: SegmentTable, paths, info: dict, hatch_groups_fn: Optional[Callable], off_mm, pts_mm, u=None) -> np.ndarray:
    """--hatch-connect: the class of every fitted path: -1 for a subpath, 2 g + f for a hatch line of fill group g whose direction d in mm has
    f = 0 iff |d . u| >= |d . n|, n = (-u_y, u_x); u = (1, 0) unless the hatch runs at an angle"""
    cls = np.full(table.n_sub, -1, np.int64)
    seg = int(info["hatch"]["segments"]) if "hatch" in info else 0
    if seg:
        groups = np.asarray(hatch_groups_fn(paths, seg), np.int64).reshape(-1)
        off_mm = np.asarray(off_mm, np.int64).reshape(-1); pts_mm = np.asarray(pts_mm, np.float64).reshape(-1, 2)
        if len(groups) != seg or (groups < 0).any() or len(off_mm) != table.n_sub + seg + 1 or (np.diff(off_mm[table.n_sub:]) != 2).any() or int(off_mm[-1]) != len(pts_mm):
            raise RuntimeError(f"{len(groups)} fill groups for {seg} hatch lines of two points each")
        a = off_mm[table.n_sub:-1]
        d = pts_mm[a + 1] - pts_mm[a]
        ux, uy = (1.0, 0.0) if u is None else (float(u[0]), float(u[1]))
        across = np.abs(d[:, 0] * ux + d[:, 1] * uy) < np.abs(d[:, 1] * ux - d[:, 0] * uy)
        cls = np.concatenate([cls, 2 * groups + across])
    return cls


def resolved_pens(pens: np.ndarray, o: SvgOptions) -> np.ndarray:
    """the pens as the G-code names them: --color-index where none was matched"""
    if not (0 <= int(o.color_index) < GC.MAX_PENS):
        raise ValueError("color index 0..7")
    return np.where(pens < 0, int(o.color_index), pens)


def hatch_angle_report(info: dict) -> str:
    """what the report lines add with --hatch-angle-deg: the angle the hatch really takes, its direction and the collapsed segments"""
    if "hatch_u" not in info:
        return ""
    u = info["hatch_u"]
    return ", {} collapsed, at {:.4f} deg (u = ({}, {}))".format(info["hatch"]["collapsed"], hatch_effective_angle(u), u[0], u[1])


def hatch_paths(table: SegmentTable, prm: dict, paths, hatch_fn, info: dict, tm: Optional[dict] = None):
    """the fitted paths with the hatch lines of the table's fill groups behind them; info["hatch"] = the counts"""
    import time
    t0 = time.perf_counter()
    fg = np.full(table.n_sub, -1, np.int32) if table.fill_group is None else np.asarray(table.fill_group, np.int32).reshape(-1)
    if len(fg) != table.n_sub:
        raise ValueError(f"fill_group has {len(fg)} entries for {table.n_sub} subpaths")
    paths, st = hatch_fn(paths, fg, prm)
    info["hatch"] = {k: int(st[k]) for k in ("groups", "lines", "crossings", "segments") + (("collapsed",) if "u" in prm else ())}
    if "u" in prm:
        info["hatch_u"] = tuple(int(v) for v in prm["u"])
    if tm is not None:
        tm["hatch"] = tm.get("hatch", 0.0) + (time.perf_counter() - t0)
    return paths


def build_stream_from_svg(text: Union[str, bytes, SegmentTable], opts: Optional[SvgOptions] = None, device=None, *, flatten_fn: Optional[Callable] = None,
                          bbox_fn: Optional[Callable] = None, fit_fn: Optional[Callable] = None, hatch_fn: Optional[Callable] = None, fetch_fn: Optional[Callable] = None,
                          steps_fn: Optional[Callable] = None, order_fn: Optional[Callable] = None, codes_fn: Optional[Callable] = None, pack_fn: Optional[Callable] = None, timings: Optional[dict] = None,
                          want_paths: bool = False, hatch_groups_fn: Optional[Callable] = None, source_fn: Optional[Callable] = None,
                          order_pens_fn: Optional[Callable] = None, merge_fn: Optional[Callable] = None, improve_fn: Optional[Callable] = None,
                          clip_fn: Optional[Callable] = None, simplify_fn: Optional[Callable] = None, dedup_fn: Optional[Callable] = None,
                          occlude_fn: Optional[Callable] = None, dash_fn: Optional[Callable] = None, seam_fn: Optional[Callable] = None,
                          hatch_link_fn: Optional[Callable] = None, stipple_fn: Optional[Callable] = None, ring_entry_fn: Optional[Callable] = None) -> Tuple[bytes, dict]:
    """The stream of an SVG text (or of a parsed SegmentTable).  Device steps, each None = the GPU (there is no CPU path in the product):
      flatten_fn(table, tol_raw) -> paths          orip_svg_flatten      (`paths` is whatever the other steps take: on the GPU a count, the points stay there)
      bbox_fn(paths) -> (min x, min y, max x, max y)   orip_svg_bbox
      fit_fn(paths, sx, sy, ox, oy) -> paths       orip_svg_fit
      hatch_fn(paths, fill_group, params) -> (paths, counts)   orip_svg_hatch  (only with --hatch-spacing-mm; params: hatch_params(); info["hatch"] = counts)
      fetch_fn(paths, with_points) -> (off int64, pts float64 or None)   orip_svg_paths_fetch  (the points only with want_paths: info["fitted_paths"])
    and the steps of the stroke driver, whose signatures and places orip.gcode.PASSES states once; steps_fn, clip_fn, hatch_link_fn, occlude_fn and stipple_fn
    take the fitted paths, where they are, in front of the arguments stated there (steps_fn and clip_fn in the place of off, pts_mm):
      steps_fn, order_fn, codes_fn, pack_fn        always
      hatch_groups_fn(paths, segments) -> int32 [segments]   orip_svg_hatch_groups_fetch  (the fill group of every hatch line), source_fn, order_pens_fn
                                                   only with --pen-colors or --allow-reverse
      merge_fn          only with --merge-paths (hatch lines go through it like any path; serpentine lines do not touch)
      improve_fn        only with --improve-order
      clip_fn           only with --clip, in the place of steps_fn (hatch lines are cut like any path, and their pens still come through the sources)
      simplify_fn       only with --simplify-mm (a hatch line has two points and passes through untouched)
      dedup_fn          only with --dedup (hatch lines go through it like any path)
      occlude_fn        only with --occlude; it needs source_fn and, with hatching, hatch_groups_fn.  The rings are the fitted paths ring_sub with their
                        levels, clamp = not --clip; info["occlude"] = the ten counts of include/orip.h.
      dash_fn           only with --dashes on a drawing that states a dash array; it needs source_fn; the patterns are dash_patterns()'s.  info["dash"] =
                        the eight counts of include/orip.h and "ignored", the dash arrays that left their stroke solid (where no stroke is dashed,
                        "ignored" alone, if any).
      hatch_link_fn     only with --hatch-connect; it needs source_fn, hatch_groups_fn and the points of fetch_fn.  The rings are the fitted paths ring_sub
                        with their fill groups, clamp = not --clip; info["hatch_link"] = the eight counts of include/orip.h and "reach".
      stipple_fn        only with --stipple-mm (with --pen-colors the dots take hatch_pens' pen of their shape).  The rings as hatch_link_fn's, rect = the
                        sheet or the clip rectangle; info["stipple"] = the seven counts of include/orip.h with the lattice, info["taps"] = the dots drawn.
      seam_fn           only with --loop-start (a circle, a <rect> and a closed <path> are closed strokes; hatch lines are open)
      ring_entry_fn     only with --ring-entry (the dots of --stipple-mm are open strokes of one point)
    With --pen-colors, info["path_pens"] is the pen of every fitted path (hatch lines included, --color-index where no stroke is stated).
    Returns (bytes, info)."""
    import time
    o = opts if opts is not None else SvgOptions()
    tm = timings if timings is not None else {}
    t0 = time.perf_counter()
    hp = hatch_params(o)
    reach = hatch_connect_reach(o)
    sp = stipple_params(o)
    if o.pen_colors is not None:
        parse_pen_colors(o.pen_colors)                      # a bad list ends the run before anything is parsed
    go = gcode_options(o)
    GC.stroke_options(go)
    table = text if isinstance(text, SegmentTable) else parse_svg(text, o.hatch_fill)
    tm["parse_svg"] = tm.get("parse_svg", 0.0) + (time.perf_counter() - t0)
    GC.apply_speed_scale(GC.GcodeOptions(speed_scale=go.speed_scale))
    tolerance_mm(o)
    info = {"segments": table.n_seg, "subpaths": table.n_sub, "canvas_height": table.canvas_height}
    if table.n_seg == 0:
        data, ginfo = GC.build_stream_from_gcode((np.zeros(1, np.int64), np.zeros((0, 2))), go)
        if want_paths:
            info["fitted_paths"] = (np.zeros(1, np.int64), np.zeros((0, 2)))
        return data, dict(ginfo, **info)
    pens_on = o.pen_colors is not None
    own = any(f is None for f in (flatten_fn, bbox_fn, fit_fn, fetch_fn)) or (hp and hatch_fn is None) or ((pens_on or o.occlude or reach is not None) and hp and hatch_groups_fn is None)
    rings = occlusion_rings(table) if o.occlude else None   # the rings and their levels are known now; the strokes' levels once the hatch lines are there
    if own:                                                 # steps of this door's own; the stroke steps are resolved by the stroke driver, once the fit says whether a dash pass runs
        if device is None:
            from .stages import device as _default_device
            device = _default_device()
        R = _Resident(device)
        flatten_fn = flatten_fn or R.flatten; bbox_fn = bbox_fn or R.bbox; fit_fn = fit_fn or R.fit; fetch_fn = fetch_fn or R.fetch
        hatch_fn = hatch_fn or R.hatch; hatch_groups_fn = hatch_groups_fn or R.hatch_groups
    paths, fi = fit_paths(table, o, flatten_fn, bbox_fn, fit_fn, tm)
    info.update(fi)
    if hp:
        paths = hatch_paths(table, hp, paths, hatch_fn, info, tm)
    pens = path_pens(table, o, paths, info, hatch_groups_fn)
    if pens is not None:
        info["path_pens"] = resolved_pens(pens, o)
    t0 = time.perf_counter()
    off_mm, pts_mm = fetch_fn(paths, want_paths or reach is not None)       # the hatch link reads a line's family off its direction
    off_mm = np.asarray(off_mm, np.int64)
    if want_paths:
        info["fitted_paths"] = (off_mm, np.asarray(pts_mm, np.float64).reshape(-1, 2))
    tm["fetch_paths"] = tm.get("fetch_paths", 0.0) + (time.perf_counter() - t0)

    def on_paths(fn, skip=0):
        """a step of this door in the stroke driver's form: the fitted paths, where they are, in front of its arguments (skip: the leading arguments of the
        driver's form that this door's has not -- off, pts_mm of the conversion)"""
        return None if fn is None else lambda *a: fn(paths, *a[skip:])
    occ = GC.Occlude(path_levels(table, paths, info, hatch_groups_fn), *rings, not o.clip) if o.occlude else None
    dsh, ignored = None, 0
    if o.dashes and table.dash_array is not None:           # the fit is known now, and with it whether any stroke is dashed: the residency rule needs to know
        pattern, phase, pat_off, pat_val, ignored = dash_patterns(table, info["scale"], o.steps_per_mm, len(off_mm) - 1)
        if (pattern >= 0).any():                            # no usable dash array: no pass, no device call
            dsh = GC.Dash(pattern, phase, pat_off, pat_val)
    lnk = None
    if reach is not None:
        lnk = GC.HatchLink(hatch_classes(table, paths, info, hatch_groups_fn, off_mm, pts_mm, hp.get("u")), *hatch_link_rings(table), not o.clip, reach)
    stp = None
    if sp is not None:
        W, H = GC.target_size(go)
        stp = GC.Stipple(*hatch_link_rings(table), not o.clip, sp["lattice"], sp["inset"], GC.clip_rect(go) or (0, 0, W - 1, H - 1),
                         (0 if o.no_serpentine else GC.STIPPLE_SERPENTINE) | (GC.STIPPLE_OCCLUDE if o.occlude else 0),
                         (lambda groups: hatch_pens(table, groups, info["pen_colors"])) if pens_on else None)
    fn = dict(convert=on_paths(clip_fn if o.clip else steps_fn, 2), hatch_link=on_paths(hatch_link_fn), occlude=on_paths(occlude_fn), stipple=on_paths(stipple_fn),
              dash=dash_fn, dedup=dedup_fn, merge=merge_fn, simplify=simplify_fn, order=order_fn, order_pens=order_pens_fn, ring_entry=ring_entry_fn, improve=improve_fn,
              seam=seam_fn, source=source_fn, codes=codes_fn, pack=pack_fn)
    data, ginfo = GC.stroke_stream((off_mm, np.zeros((int(off_mm[-1]), 2))), go, device, GC.StrokeSteps(fn, dsh, lnk, occ, stp), tm, pens, force=bool(own),
                                   convert=lambda dev: on_paths(_Resident(dev).clip if o.clip else _Resident(dev).steps, 2))
    if "dash" in ginfo or ignored:                          # an ignored dash array is reported whether or not a pass ran: the stroke is solid, and the line says so
        ginfo["dash"] = dict(ginfo.get("dash", {}), ignored=ignored)
    return data, dict(ginfo, **info)


# ------------------------------------------------------------------ command lines
def _add_fit_args(ap: argparse.ArgumentParser, d: SvgOptions):
    ap.add_argument("--page-width-mm", type=float, default=d.page_width_mm, help="target page width in mm (default: 210, A4)")
    ap.add_argument("--page-height-mm", type=float, default=d.page_height_mm, help="target page height in mm (default: 297, A4)")
    ap.add_argument("--margin-mm", type=float, default=d.margin_mm, help="margin from the page border in mm (default: 10)")
    ap.add_argument("--scale", type=float, default=None, help="uniform scale, SVG units -> mm; overrides the automatic fit")
    ap.add_argument("--scale-x", type=float, default=None, help="X scale; overrides --scale for X")
    ap.add_argument("--scale-y", type=float, default=None, help="Y scale; overrides --scale for Y")
    ap.add_argument("--tolerance-mm", type=float, default=None, help="largest distance between a curve and its polyline on the page (default: half a step, 0.5 / steps per mm)")
    ap.add_argument("--hatch-spacing-mm", type=float, default=None, help="hatch-fill closed shapes with lines this far apart (default: no hatching); rounded to whole steps")
    ap.add_argument("--hatch-inset-mm", type=float, default=d.hatch_inset_mm, help="how far each hatch line stays inside the outline (default: 0.675, 27 steps at 40 steps per mm)")
    ap.add_argument("--hatch-direction", choices=sorted(HATCH_DIRECTIONS), default=d.hatch_direction, help="hatch lines along X, along Y, or both (default: horizontal); with "
                                                                                                          "--hatch-angle-deg: along the angle, across it, or both")
    ap.add_argument("--hatch-angle-deg", type=float, default=None, help="hatch along this angle, counter-clockwise in the frame of the written G-code (before --invert-y), exact on "
                                                                         "the step grid, one family of lines for the whole drawing (default: the reference's hatch along X / Y)")
    ap.add_argument("--no-serpentine", action="store_true", help="draw every hatch line in the same direction; by default every other line is reversed")
    ap.add_argument("--hatch-fill", choices=HATCH_FILLS, default=d.hatch_fill, help="stated: elements whose fill is written down and is not none (default); all: every element that draws")
    ap.add_argument("--pen-colors", default=None, help="the colour of each pen, comma-separated (#rgb, #rrggbb or a keyword; position = pen), or rgbk; a path is drawn with the pen "
                                                        "nearest to its stroke colour (default: one pen, --color-index)")


def build_gcode_argparser() -> argparse.ArgumentParser:
    d = SvgOptions()
    ap = argparse.ArgumentParser(description="Convert SVG to G-code fitted onto a page; curves are flattened and fitted on the GPU.")
    ap.add_argument("input", help="input SVG file")
    ap.add_argument("-o", "--output", default=d.output, help="output G-code file (default: from_svg.gcode)")
    ap.add_argument("--movement-speed", type=float, default=d.movement_speed, help="accepted for the reference's command line; only matters to a laser, a pen plot has no feed words")
    ap.add_argument("--cutting-speed", type=float, default=d.cutting_speed, help="accepted for the reference's command line; only matters to a laser")
    ap.add_argument("--passes", type=int, default=d.passes, help="number of passes over the same paths (the paths are repeated)")
    ap.add_argument("--pass-depth", type=float, default=d.pass_depth, help="accepted for the reference's command line; only matters to a laser")
    ap.add_argument("--steps-per-mm", type=float, default=d.steps_per_mm, help="sets the default tolerance and the grid of the hatch lines here")
    _add_fit_args(ap, d)
    return ap


def build_stream_argparser() -> argparse.ArgumentParser:
    d = SvgOptions()
    ap = argparse.ArgumentParser(description="Convert SVG directly to an OmniRevolve plotter stream and render its preview; one process, geometry on the GPU.")
    ap.add_argument("input", help="input SVG file")
    ap.add_argument("-o", "--output-stream", default=None, help="output stream file (default: <svg stem>_stream.bin)")
    ap.add_argument("--gcode-output", default=None, help="G-code output file (default: <svg stem>.gcode)")
    _add_fit_args(ap, d)
    ap.add_argument("--steps-per-mm", type=float, default=d.steps_per_mm)
    ap.add_argument("--target-width-steps", type=int, default=None, help="canvas width in steps (default: page width x steps per mm; needs the height too)")
    ap.add_argument("--target-height-steps", type=int, default=None, help="canvas height in steps (default: page height x steps per mm; needs the width too)")
    ap.add_argument("--invert-y", type=int, default=d.invert_y, help="1: flip Y inside the canvas")
    ap.add_argument("--color-index", type=int, default=d.color_index, help="pen 0..7")
    ap.add_argument("--speed-scale", type=float, default=d.speed_scale, help="> 1 faster (smaller dividers), < 1 slower")
    GC.add_stroke_args(ap, ("--no-reorder", "--pen-order", "--allow-reverse") + GC.STROKE_ARGS[3:], "; the G-code file is not changed")
    ap.add_argument("--occlude", action="store_true", help="filled shapes (what --hatch-fill marks) hide the strokes and hatch lines of the elements painted before them; "
                                                           "exact on the step grid; the G-code file is not changed")
    ap.add_argument("--loop-start", action="store_true", help="start and end every closed stroke (a circle, a rectangle, a closed path) at the vertex that makes the pen-up "
                                                              "travel of the whole plot least, all of them chosen together, after the order; the G-code file is not changed")
    ap.add_argument("--ring-entry", action="store_true", help="let the greedy order enter a closed stroke (a circle, a rectangle, a closed path) at its nearest vertex instead "
                                                              "of the one it lists first; not with --no-reorder; the G-code file is not changed")
    ap.add_argument("--dashes", action="store_true", help="draw a stroke that states a stroke-dasharray as its dashes, measured on the step grid from the start of "
                                                          "every stroke (hatch lines stay solid); the G-code file is not changed")
    ap.add_argument("--hatch-connect", action="store_true", help="draw a hatch as zigzags: join consecutive hatch lines of one shape by straight links that lie wholly "
                                                                 "inside it, so the pen stays down; needs --hatch-spacing-mm; the G-code file is not changed")
    ap.add_argument("--hatch-connect-mm", type=float, default=None, help="the longest link (default: twice --hatch-spacing-mm); needs --hatch-connect")
    ap.add_argument("--stipple-mm", type=float, default=None, help="fill the shapes --hatch-fill marks with dots (pen taps) this far apart, on one lattice for the whole "
                                                                   "drawing; rounded to whole steps; the G-code file is not changed")
    ap.add_argument("--stipple-inset-mm", type=float, default=None, help="how far every dot stays inside its shape's outline (default: 0.675, as --hatch-inset-mm); needs --stipple-mm")
    ap.add_argument("--stipple-pattern", choices=STIPPLE_PATTERNS, default=None, help="square: rows a pitch apart; stagger (default): every other row moved by half a pitch, "
                                                                                      "the rows 3547/4096 of a pitch apart; needs --stipple-mm")
    ap.add_argument("--no-preview", action="store_true", help="do not render <svg stem>_stream_preview.png")
    ap.add_argument("--preview-render-width", type=int, default=d.preview_render_width)
    ap.add_argument("--preview-render-height", type=int, default=d.preview_render_height)
    return ap


def options_from_args(a: argparse.Namespace) -> SvgOptions:
    return SvgOptions(**{f.name: getattr(a, f.name) for f in fields(SvgOptions) if hasattr(a, f.name)})


def _read(path: str) -> bytes:
    p = Path(path)
    if not p.is_file():
        raise SystemExit(f"Input SVG not found: {p}")
    return p.read_bytes()


def main_gcode(argv: Optional[Sequence[str]] = None, **device_steps) -> None:
    """svg2gcode.py: the fitted paths as G-code"""
    a = build_gcode_argparser().parse_args(argv)
    o = options_from_args(a)
    hp = hatch_params(o)
    if o.pen_colors is not None:
        parse_pen_colors(o.pen_colors)
    table = parse_svg(_read(a.input), o.hatch_fill)
    info = {}
    off, pts, pens = np.zeros(1, np.int64), np.zeros((0, 2)), None
    if table.n_seg:
        R = device_steps
        if not R:
            from .stages import device as _default_device
            r = _Resident(_default_device())
            R = dict(flatten_fn=r.flatten, bbox_fn=r.bbox, fit_fn=r.fit, fetch_fn=r.fetch, hatch_fn=r.hatch, hatch_groups_fn=r.hatch_groups)
        paths, info = fit_paths(table, o, R["flatten_fn"], R["bbox_fn"], R["fit_fn"])
        if hp:
            paths = hatch_paths(table, hp, paths, R["hatch_fn"], info)
        pens = path_pens(table, o, paths, info, R.get("hatch_groups_fn"))
        off, pts = R["fetch_fn"](paths, True)
    Path(a.output).write_text(gcode_text(off, pts, o.passes, None if pens is None else resolved_pens(pens, o)), encoding="utf-8")
    print(f"G-code saved to {a.output}: {len(off) - 1} paths, {len(pts)} points")
    if "scale" in info:
        sx, sy, ox, oy = info["scale"]
        print(f"  Raw bbox: x=[{info['bbox'][0]:.3f}, {info['bbox'][2]:.3f}], y=[{info['bbox'][1]:.3f}, {info['bbox'][3]:.3f}]")
        print(f"  Final scale: sx={sx:.5f}, sy={sy:.5f}; offsets: {ox:.3f}, {oy:.3f} mm; tolerance {tolerance_mm(o)} mm = {info['tol_raw']:.6g} raw units")
    if "hatch" in info:
        print("  Hatch: {groups} fill groups, {lines} lines, {crossings} crossings -> {segments} segments".format(**info["hatch"]) + hatch_angle_report(info))


def main_stream(argv: Optional[Sequence[str]] = None, **device_steps) -> None:
    """svg2stream.py: G-code file, stream file and (unless --no-preview) the preview PNG"""
    a = build_stream_argparser().parse_args(argv)
    o = options_from_args(a)
    src = Path(a.input)
    text = _read(a.input)
    gcode_path = Path(a.gcode_output) if a.gcode_output else src.with_suffix(".gcode")
    stream_path = Path(a.output_stream) if a.output_stream else src.with_name(src.stem + "_stream.bin")
    device = device_steps.pop("device", None)
    if device is None and not device_steps:
        from .stages import device as _default_device
        device = _default_device()
    data, info = build_stream_from_svg(text, o, device, want_paths=True, **device_steps)
    off, pts = info["fitted_paths"]
    gcode_path.write_text(gcode_text(off, pts, pens=info.get("path_pens")), encoding="utf-8")
    stream_path.write_bytes(data)
    print(f"[svg] {a.input}: {info['segments']} segments in {info['subpaths']} subpaths -> {len(pts)} points")
    if "hatch" in info:
        print("[svg] hatch: {groups} fill groups, {lines} lines, {crossings} crossings -> {segments} segments".format(**info["hatch"]) + hatch_angle_report(info))
    for line in GC.report_lines("svg", info, unmatched=True):
        print(line)
    print(f"[svg] G-code saved: {gcode_path}")
    print(f"stream saved: {stream_path} ({len(data)} bytes)")
    if o.no_preview:
        print("Preview disabled (--no-preview).")
        return
    from . import stream_preview as SP
    W, H = info["target"]
    palette = {}
    if "pen_colors" in info:                              # the pens' own colours; the previewer has four (pens 4..7 render as pen 3, as they always did)
        palette = {"palette": tuple((list(info["pen_colors"]) + list(SP.DEFAULT_PALETTE[len(info["pen_colors"]):]))[:4])}
    rgb, _ = SP.preview(device, data, W, H, o.preview_render_width, o.preview_render_height, invert_y=True, **palette)
    png = src.with_name(src.stem + "_stream_preview.png")
    SP.save_png(rgb, str(png))
    print(f"Image saved: {png}")
