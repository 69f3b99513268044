"""TEST INFRASTRUCTURE: the plain definitions behind the pens -- a brute-force numpy order (orip_gcode_order_pens as include/orip.h states it: no grid, no
cells, every remaining candidate looked at in every step), the events of a plan in the vocabulary of the reference's draw_color_group, and stand-ins for
the two small fetches (source indices of the step polylines, fill groups of the hatch lines).  Written independently of csrc/gcode.hip and pinned by
tests/golden/golden_pens.npz, which holds what the reference's own functions returned."""
import numpy as np

import gcode_double as GD
import hatch_double as HD

TRAVEL, COLOR, DOWN, LINE, UP = 0, 1, 2, 3, 4          # event codes, also those of tests/golden/make_golden_pens.py


def order_pens_numpy(ends, group, n_groups, reverse=False, start=(0, 0)):
    """-> (order int32 [n], rev bool [n]): group after group, the minimum of (L1 distance << 32) | (2 i + r) over the group's remaining paths"""
    e = np.asarray(ends, np.int64).reshape(-1, 4)
    grp = np.asarray(group, np.int64).reshape(-1)
    n = len(e)
    idx = np.arange(n, dtype=np.uint64)
    dead = np.iinfo(np.uint64).max                    # the key is unsigned: a distance of 2^31 (corner to corner of the coordinate range) still fits its high word
    order, rev = np.zeros(n, np.int32), np.zeros(n, bool)
    cx, cy = int(start[0]), int(start[1])
    k = 0

    def keys(x, y, r):
        return ((np.abs(x - cx) + np.abs(y - cy)).astype(np.uint64) << np.uint64(32)) | (np.uint64(2) * ii + np.uint64(r))
    for g in range(int(n_groups)):
        sel = np.nonzero(grp == g)[0]
        ee, ii = e[sel], idx[sel]
        alive = np.ones(len(sel), bool)
        for _ in range(len(sel)):
            key = keys(ee[:, 0], ee[:, 1], 0)
            if reverse:
                key = np.minimum(key, keys(ee[:, 2], ee[:, 3], 1))
            j = int(np.argmin(np.where(alive, key, dead)))
            r = int(key[j]) & 1
            order[k] = int(ii[j]); rev[k] = bool(r); alive[j] = False; k += 1
            cx, cy = (int(ee[j, 0]), int(ee[j, 1])) if r else (int(ee[j, 2]), int(ee[j, 3]))
    return order, rev


def plan_events(P, skip=0):
    """the items of an orip.stream.Plan behind its first `skip`, as rows (code, a, b, c, d): TRAVEL / LINE with the move's (x0, y0, x1, y1), COLOR with the
    pen in a, DOWN, UP"""
    out = []
    m = 0
    for i, k in enumerate(np.asarray(P.kind).tolist()):
        if k < 0:
            row = [TRAVEL if P.is_travel[m] else LINE, *np.asarray(P.moves[m]).tolist()]; m += 1
        elif k == 0x01: row = [UP, 0, 0, 0, 0]
        elif k == 0x02: row = [DOWN, 0, 0, 0, 0]
        elif 0x08 <= k <= 0x0F: row = [COLOR, k & 7, 0, 0, 0]
        else: row = [-1, k, 0, 0, 0]
        if i >= skip:
            out.append(row)
    return np.asarray(out, np.int64).reshape(-1, 5)


class StepsWithSource:
    """gcode_double.to_steps_numpy that also remembers which input path every step polyline came from (orip_gcode_steps_source_fetch)"""
    def __init__(self): self.src = np.zeros(0, np.int32)

    def steps(self, off, pts_mm, m):
        off = np.asarray(off, np.int64)
        out_off, out_pts = GD.to_steps_numpy(off, pts_mm, m)
        # a path survives iff it keeps two points: convert each alone (the definition, not the fast way)
        keep = []
        p = np.asarray(pts_mm, np.float64).reshape(-1, 2)
        for i in range(len(off) - 1):
            o1, _ = GD.to_steps_numpy(np.array([0, off[i + 1] - off[i]]), p[off[i]:off[i + 1]], m)
            if len(o1) == 2:
                keep.append(i)
        self.src = np.asarray(keep, np.int32)
        assert len(self.src) == len(out_off) - 1
        return out_off, out_pts

    def source(self, n):
        assert n == len(self.src)
        return self.src


class HatchWithGroups:
    """hatch_double.hatch_numpy that also remembers the fill group of every hatch line (orip_svg_hatch_groups_fetch): per direction, horizontal first, the
    groups ascending, each with as many lines as hatching that group ALONE gives"""
    def __init__(self): self.groups = np.zeros(0, np.int32)

    def hatch(self, paths, fill_group, prm):
        from orip.lib import HATCH_HORIZONTAL, HATCH_VERTICAL, HATCH_SERPENTINE
        out, st = HD.hatch_numpy(paths, fill_group, prm)
        off, q = np.asarray(paths[0], np.int64), HD.quantise(paths[1], prm["steps_per_mm"])
        fg = np.asarray(fill_group, np.int64)
        groups = []
        for d in (HATCH_HORIZONTAL, HATCH_VERTICAL):
            if prm["flags"] & d:
                for g in np.unique(fg[fg >= 0]).tolist():
                    seg, _ = HD.hatch_segments(off, q, np.where(fg == g, g, -1), prm["spacing"], prm["inset"], d | (prm["flags"] & HATCH_SERPENTINE))
                    groups += [g] * len(seg)
        self.groups = np.asarray(groups, np.int32)
        assert len(self.groups) == st["segments"]
        return out, st

    def hatch_groups(self, paths, segments):
        assert segments == len(self.groups)
        return self.groups


def pens_doubles():
    """the keyword arguments that put every device step of orip.svg.build_stream_from_svg on the CPU, those of the pens included"""
    import svg_double as SD
    S, H = StepsWithSource(), HatchWithGroups()
    return dict(SD.svg_doubles(), steps_fn=lambda paths, m: S.steps(paths[0], paths[1], m), source_fn=S.source, hatch_fn=H.hatch, hatch_groups_fn=H.hatch_groups,
                order_pens_fn=lambda ends, group, n_groups, reverse: order_pens_numpy(ends, group, n_groups, reverse))


# the drawing of the whole-tool tests: three stroke colours (red twice, through a group; green in a style property and as #0f0; blue by keyword), a shape filled
# black under a blue outline, and a rectangle that states no stroke
TOOL_SVG = b"""<svg xmlns="http://www.w3.org/2000/svg" width="200" height="200" viewBox="0 0 200 200">
 <g stroke="#f00"><path d="M10 10 L90 10 L90 60"/><line x1="20" y1="30" x2="60" y2="80"/></g>
 <path style="stroke: rgb(0, 255, 0); fill:none" d="M100 20 C120 0 160 40 180 20"/>
 <polyline stroke="Blue" fill="none" points="20,120 60,160 100,120 140,160"/>
 <circle cx="150" cy="110" r="30" fill="black" stroke="#00f"/>
 <rect x="30" y="170" width="60" height="20"/>
 <path stroke="#0f0" d="M180 180 L120 190"/>
</svg>
"""
TOOL_PLAIN_ARGS = ["--hatch-spacing-mm", "1.0"]                      # options the tool had before the pens
TOOL_PEN_ARGS = TOOL_PLAIN_ARGS + ["--pen-colors", "rgbk", "--allow-reverse"]
