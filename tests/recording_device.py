"""TEST INFRASTRUCTURE: a stand-in for orip.device.Device on the CPU, for the host driver of the vector front doors (orip/gcode.py, orip/svg.py).  Every
method the driver reaches is here, computed by the numpy doubles of tests/*_double.py, and -- the point of it -- with state of its own, as the device has:
the resident step polylines, their source table, the fitted (or flattened) paths in mm, the fill groups of the hatch lines and the direction codes.  A
call in the resident form (off is None) computes from what the stand-in holds and not from what the host holds, and raises when `n` is not the number of
polylines it holds; an uploaded list replaces what it holds.  So a driver that takes the resident form where the list on the host is another one gets other
bytes or an error, and one that uploads where it need not is seen in `log`: one (method, "resident" | "uploaded") entry per call, "resident" for a call
that reads the stroke list (or, svg_*, the fitted paths) the stand-in holds, "uploaded" for one that is sent its input.

The sources follow as include/orip.h states: through origin (dash, occlusion, dedup), through the first member (hatch link), unchanged through the
simplification, gone behind a merge and behind an uploaded list of another count than the resident one."""
import numpy as np


class ResidencyError(RuntimeError):
    """a call asked for resident data the stand-in does not hold, or for another count of it"""


def _ends(off, pts):
    return np.ascontiguousarray(np.concatenate([pts[off[:-1]], pts[off[1:] - 1]], 1), np.int32)


class RecordingDevice:
    def __init__(self):
        self.log = []
        self.strokes = None         # (off int64, pts int32): the resident step polylines
        self.src = None             # the input path of every resident polyline, or None: no sources
        self.convert_src = None     # the same as the last conversion left it
        self.fitted = None          # (off int64, pts float64): the resident paths in mm
        self.groups = None          # the fill group of every hatch line
        self.codes = None

    def close(self):
        pass

    # ---- state
    def _read(self, method, off, pts, n, rewrites=True):
        """the stroke list a pass works on: the resident one (off is None, n must be its count) or the uploaded one (rewrites: the pass leaves a new list)"""
        if off is None:
            if pts is not None or self.strokes is None or n is None or int(n) != len(self.strokes[0]) - 1:
                raise ResidencyError(f"{method}: {n} resident polylines asked for, {None if self.strokes is None else len(self.strokes[0]) - 1} held")
            self.log.append((method, "resident"))
            return self.strokes
        self.log.append((method, "uploaded"))
        off = np.asarray(off, np.int64).reshape(-1); pts = np.asarray(pts, np.int32).reshape(-1, 2)
        if rewrites and (self.strokes is None or len(off) != len(self.strokes[0])):
            self.src = None
        return off, pts

    def _keep(self, off, pts, src):
        self.strokes = (np.asarray(off, np.int64).reshape(-1), np.asarray(pts, np.int32).reshape(-1, 2)); self.src = src

    def _fitted(self, method, n=None):
        if self.fitted is None or (n is not None and int(n) != len(self.fitted[0]) - 1):
            raise ResidencyError(f"{method}: {n} resident paths in mm asked for, {None if self.fitted is None else len(self.fitted[0]) - 1} held")
        return self.fitted

    def _mm(self, method, off, pts_mm, n):
        if off is None:
            self.log.append((method, "resident"))
            return self._fitted(method, n)
        self.log.append((method, "uploaded"))
        return np.asarray(off, np.int64), np.asarray(pts_mm, np.float64).reshape(-1, 2)

    def _rings(self, method, ring_sub, m, clamp):
        import occlude_double as OD
        off, pts = self._fitted(method)
        return OD.rings_to_steps(off, pts, np.asarray(ring_sub).tolist(), m, clamp)

    # ---- conversion, sources
    def gcode_to_steps(self, off, pts_mm, map, fetch_points=True, n=None):
        import pens_double as PD
        S = PD.StepsWithSource()
        o, p = S.steps(*self._mm("gcode_to_steps", off, pts_mm, n), map)
        self._keep(o, p, np.asarray(S.src, np.int64)); self.convert_src = self.src
        return self.strokes

    def gcode_to_steps_clip(self, off, pts_mm, map, rect, n=None):
        import clip_double as CD
        o, p, src, st = CD.clip_numpy(*self._mm("gcode_to_steps_clip", off, pts_mm, n), map, rect)
        self._keep(o, p, np.asarray(src, np.int64)); self.convert_src = self.src
        return (*self.strokes, st)

    def gcode_steps_source(self, n):
        self.log.append(("gcode_steps_source", "resident"))
        if self.src is None or len(self.src) != int(n):
            raise ResidencyError(f"gcode_steps_source: {n} sources asked for, {None if self.src is None else len(self.src)} held")
        return self.src.astype(np.int32)

    # ---- paths in mm
    def gcode_flatten(self, table, tol):
        import arc_double as AD
        self.log.append(("gcode_flatten", "uploaded"))
        off, pts, st = AD.flatten(table, tol)
        self.fitted = (off, pts)
        return len(pts), st

    def svg_flatten(self, table, tol):
        import svg_double as SD
        self.log.append(("svg_flatten", "uploaded"))
        off, pts = SD.flatten_numpy(table, tol)
        self.fitted = (np.asarray(off, np.int64), np.asarray(pts, np.float64).reshape(-1, 2))
        return len(self.fitted[1])

    def svg_paths(self, n=None, with_points=True):
        self.log.append(("svg_paths", "resident"))
        off, pts = self._fitted("svg_paths", n)
        return off.copy(), (pts.copy() if with_points else None)

    def svg_bbox(self):
        import svg_double as SD
        return SD.bbox_numpy(self._fitted("svg_bbox"))

    def svg_fit(self, sx, sy, ox, oy):
        import svg_double as SD
        off, pts = SD.fit_numpy(self._fitted("svg_fit"), sx, sy, ox, oy)
        self.fitted = (np.asarray(off, np.int64), pts)

    def _hatch(self, H, fill_group, prm):
        (off, pts), st = H.hatch(self._fitted("svg_hatch"), np.asarray(fill_group), prm)
        self.fitted = (np.asarray(off, np.int64), np.asarray(pts, np.float64).reshape(-1, 2)); self.groups = np.asarray(H.groups, np.int32)
        return st

    def svg_hatch(self, fill_group, steps_per_mm, spacing, inset, flags):
        import pens_double as PD
        return self._hatch(PD.HatchWithGroups(), fill_group, dict(steps_per_mm=steps_per_mm, spacing=spacing, inset=inset, flags=flags))

    def svg_hatch_angle(self, fill_group, steps_per_mm, spacing, inset, u, flags):
        import hatch_angle_double as HA
        return self._hatch(HA.HatchAngleWithGroups(), fill_group, dict(steps_per_mm=steps_per_mm, spacing=spacing, inset=inset, u=u, flags=flags))

    def svg_hatch_groups(self, segments):
        if self.groups is None or len(self.groups) != int(segments):
            raise ResidencyError(f"svg_hatch_groups: {segments} hatch lines asked for, {None if self.groups is None else len(self.groups)} held")
        return self.groups

    # ---- the passes that rewrite the stroke list
    def _cut(self, out):
        off, pts, origin, st = out
        self._keep(off, pts, None if self.src is None else self.src[np.asarray(origin, np.int64)])
        return (*self.strokes, np.asarray(origin, np.int32), st)

    def gcode_dash(self, off, pts, pattern, phase, pat_off, pat_val, n=None):
        import dash_double as DH
        return self._cut(DH.dash_numpy(*self._read("gcode_dash", off, pts, n), pattern, phase, pat_off, pat_val))

    def gcode_dedup(self, off, pts, group, n_groups, n=None):
        import dedup_double as DD
        return self._cut(DD.dedup_numpy(*self._read("gcode_dedup", off, pts, n), group, n_groups))

    def gcode_occlude(self, off, pts, level, ring_off, ring_pts, ring_level, n=None):
        import occlude_double as OD
        return self._cut(OD.occlude_numpy(*self._read("gcode_occlude", off, pts, n), level, ring_off, ring_pts, ring_level))

    def svg_occlude(self, level, ring_sub, ring_level, map, clamp, n=None):
        import occlude_double as OD
        return self._cut(OD.occlude_numpy(*self._read("svg_occlude", None, None, n), level, *self._rings("svg_occlude", ring_sub, map, clamp), ring_level))

    def _link(self, out):
        off, pts, member_off, member, st = out
        first = np.asarray(member, np.int64)[np.asarray(member_off, np.int64)[:-1]]
        self._keep(off, pts, None if self.src is None else self.src[first])
        return (*self.strokes, np.asarray(member_off, np.int64), np.asarray(member, np.int32), st)

    def gcode_hatch_link(self, off, pts, cls, ring_off, ring_pts, ring_group, reach, n=None):
        import hatch_link_double as LD
        return self._link(LD.hatch_link(*self._read("gcode_hatch_link", off, pts, n), cls, ring_off, ring_pts, ring_group, reach))

    def svg_hatch_link(self, cls, ring_sub, ring_group, map, clamp, reach, n=None):
        import hatch_link_double as LD
        return self._link(LD.hatch_link(*self._read("svg_hatch_link", None, None, n), cls, *self._rings("svg_hatch_link", ring_sub, map, clamp), ring_group, reach))

    def gcode_merge(self, off, pts, group, n_groups, reverse=False, n=None):
        import merge_double as MD
        out = MD.merge_numpy(*self._read("gcode_merge", off, pts, n), group, n_groups, reverse)
        self._keep(out[0], out[1], None)
        return (*self.strokes, *out[2:])

    def gcode_simplify(self, off, pts, tol4, n=None):
        import simplify_double as SP
        out = SP.simplify_numpy(*self._read("gcode_simplify", off, pts, n), tol4)
        self._keep(out[0], out[1], self.src)
        return (*self.strokes, *out[2:])

    # ---- the passes that read it
    def svg_stipple(self, ring_sub, ring_group, map, clamp, lattice, inset, rect, flags):
        import stipple_double as SD
        self.log.append(("svg_stipple", "resident"))
        return SD.stipple(*self._rings("svg_stipple", ring_sub, map, clamp), ring_group, lattice, inset, rect, flags)

    def _read_ends(self, method, ends, n):
        if ends is None:
            return _ends(*self._read(method, None, None, n, False))
        self.log.append((method, "uploaded"))
        return np.asarray(ends, np.int32).reshape(-1, 4)

    def gcode_order(self, ends, n=None):
        import gcode_double as D
        return D.order_numpy(self._read_ends("gcode_order", ends, n))

    def gcode_order_pens(self, ends, group, n_groups, reverse=False, start=(0, 0), n=None):
        import pens_double as PD
        return PD.order_pens_numpy(self._read_ends("gcode_order_pens", ends, n), group, n_groups, reverse, start)

    def gcode_improve(self, ends, group, n_groups, order, rev, reverse=False, start=(0, 0), max_rounds=None, n=None):
        import improve_double as ID
        return ID.improve(self._read_ends("gcode_improve", ends, n), group, n_groups, order, rev, reverse, start, max_rounds)

    def gcode_seam(self, off, pts, order, rev, start=(0, 0), n=None):
        import seam_double as SM
        return SM.seams(*self._read("gcode_seam", off, pts, n, False), order, rev, start)

    def gcode_order_rings(self, off, pts, group, n_groups, reverse=False, start=(0, 0), n=None):
        import ring_entry_double as RD
        return RD.order_rings(*self._read("gcode_order_rings", off, pts, n, False), group, n_groups, reverse, start)

    # ---- the stream compiler
    def stream_codes(self, moves, fetch_codes=True):
        from stream_double import codes_numpy
        off, self.codes = codes_numpy(moves)
        return off, (self.codes if fetch_codes else None)

    def stream_pack(self, table, codes=None):
        import gcode_double as D
        if codes is not None or self.codes is None:
            raise ResidencyError("stream_pack reads the codes stream_codes left resident")
        return D.pack_numpy(table, self.codes)


# ------------------------------------------------------------------ runs in which some passes are given and the others are the device's own
# the factors of such a run, in pipeline order, and the step keywords of the front doors that give each; "source" is source_fn, not a pass
KEYWORDS = {"flatten": ("flatten_fn",), "convert": ("steps_fn", "clip_fn"), "source": ("source_fn",), "dash": ("dash_fn",), "hatch_link": ("hatch_link_fn",),
            "occlude": ("occlude_fn",), "dedup": ("dedup_fn",), "merge": ("merge_fn",), "simplify": ("simplify_fn",), "stipple": ("stipple_fn",),
            "order": ("order_fn", "order_pens_fn", "ring_entry_fn"), "improve": ("improve_fn",), "seam": ("seam_fn",)}
SVG_FRONT = ("flatten_fn", "bbox_fn", "fit_fn", "fetch_fn", "hatch_fn", "hatch_groups_fn")      # always the device's own in a mixed run: the fitted paths live there


def factors_on(door, row, arcs=False):
    """the factors of KEYWORDS a row of compose_cases (a dict of levels) switches on, in pipeline order"""
    import compose_cases as CC
    grouped = bool(row["pens"] or row["reverse"])
    on = {"flatten": arcs, "convert": True, "source": grouped or bool(row["dash"] or row.get("connect") or row.get("occlude")), "dash": bool(row["dash"]),
          "hatch_link": bool(row.get("connect")), "occlude": bool(row.get("occlude")), "dedup": bool(row["dedup"]), "merge": bool(row["merge"]),
          "simplify": bool(row["simplify"]), "stipple": bool(row.get("stipple")), "order": row["order"] != CC.NO_REORDER, "improve": bool(row["improve"]),
          "seam": bool(row["loop"])}
    return [name for name in KEYWORDS if on[name]]


def coherent(given):
    """the device's sources are those of its own conversion: behind a given conversion the sources are given too"""
    return not (given.get("convert") and given.get("source") is False)


def assignments(names, seed=20240):
    """the given / own assignments of a run over the factors `names`, each a dict name -> True (given): all own, the two that alternate strictly (source_fn
    is given wherever that would ask a device for the sources of a given conversion), and a strength-2 covering array over the factors as binary ones,
    greedy from a seeded generator as compose_cases.generate_rows builds its rows.  Without repeats, in that order."""
    import itertools
    rng = np.random.default_rng(seed)

    def mended(a):
        return a if coherent(a) else dict(a, source=True)
    out = [{n: False for n in names}] + [mended({n: (i + k) % 2 == 0 for i, n in enumerate(names)}) for k in (0, 1)]
    need = {frozenset(((a, x), (b, y))) for a, b in itertools.combinations(names, 2) for x in (False, True) for y in (False, True) if coherent({a: x, b: y})}

    def covered(a):
        return {frozenset(((p, a[p]), (q, a[q]))) for p, q in itertools.combinations(names, 2)}
    for a in out:
        need -= covered(a)
    while need:
        pending = sorted(need, key=lambda t: sorted(t))
        best, gain = None, -1
        for _ in range(48):
            cand = dict(pending[int(rng.integers(len(pending)))])
            for n in names:
                cand.setdefault(n, bool(rng.integers(2)))
            cand = {n: cand[n] for n in names}
            g = len(covered(cand) & need) if coherent(cand) else -1
            if g > gain:
                best, gain = cand, g
        out.append(best); need -= covered(best)
    return [a for i, a in enumerate(out) if a not in out[:i]]


def given_steps(door, dev, angle=False):
    """every step keyword of KEYWORDS for a door, as the numpy doubles of compose_cases, fit for a run in which other steps are `dev`'s own: a given step
    of the SVG door reads the fitted paths where the device holds them (dev.svg_paths()), and source_fn gives the sources as the conversion left them --
    the given conversion's, or, behind the device's own, what the device says when first asked (before any pass has moved them on).  A new set per run."""
    import compose_cases as CC
    ran, first = [], {}

    def noting(fn):
        def call(*a):
            ran.append(1)
            return fn(*a)
        return call
    if door == "svg":
        d = {k: v for k, v in CC.svg_doubles_all(angle).items() if k not in SVG_FRONT}
        for k in ("steps_fn", "clip_fn", "occlude_fn", "hatch_link_fn", "stipple_fn"):
            d[k] = (lambda fn: lambda _paths, *a: fn(dev.svg_paths(), *a))(d[k])
    else:
        import arc_double as AD
        d = dict(CC.gcode_doubles_all(), flatten_fn=AD.flatten_fn)
    d["steps_fn"], d["clip_fn"], converted = noting(d["steps_fn"]), noting(d["clip_fn"]), d["source_fn"]

    def source(n):
        if ran:
            return converted(n)
        if "src" not in first:
            first["src"] = np.array(dev.gcode_steps_source(n))
        assert len(first["src"]) == n
        return first["src"]
    d["source_fn"] = source
    return d


def run_mixed(door, options, text, given, dev, angle=False):
    """(bytes, info) of a front door with the factors named in `given` (a dict name -> bool, or the names) given and every other step dev's own"""
    steps = given_steps(door, dev, angle)
    kw = {k: steps[k] for name in KEYWORDS if (given.get(name) if isinstance(given, dict) else name in given) for k in KEYWORDS[name] if k in steps}
    if door == "svg":
        from orip import svg as SV
        return SV.build_stream_from_svg(text, options, dev, **kw)
    from orip import gcode as GC
    return GC.build_stream_from_gcode(text, options, dev, **kw)


# ------------------------------------------------------------------ the step keywords of the front doors against the pass table
PIPELINE = ("flatten", "convert", "dash", "hatch_link", "occlude", "dedup", "merge", "simplify", "stipple", "order", "ring_entry", "improve", "seam")
SVG_FRONT_STEPS = ("flatten_fn", "bbox_fn", "fit_fn", "hatch_fn", "fetch_fn", "hatch_groups_fn")      # the SVG door's steps in front of the stroke driver


def step_keywords(door):
    """the *_fn keywords a front door accepts, read off its signature"""
    import inspect
    from orip import gcode as GC, svg as SV
    sig = inspect.signature(SV.build_stream_from_svg if door == "svg" else GC.build_stream_from_gcode)
    return {k for k, p in sig.parameters.items() if k.endswith("_fn") and p.kind is p.KEYWORD_ONLY}


def doors_take_the_pass_table():
    """holds the doors to orip.gcode.PASSES: the table is in pipeline order, each door accepts exactly the step keywords the table and the steps beside it
    state, and the G-code door's lack the three SVG-only ones -> (the G-code door's step keywords, the SVG door's)"""
    from orip import gcode as GC
    table = {k for p in GC.PASSES for k in p.keywords} | set(GC.OTHER_STEPS)
    assert tuple(p.name for p in GC.PASSES) == PIPELINE
    assert set(GC.SVG_ONLY_STEPS) == {"hatch_link_fn", "occlude_fn", "stipple_fn"} <= table
    assert step_keywords("gcode") == table - set(GC.SVG_ONLY_STEPS) and step_keywords("svg") == table | set(SVG_FRONT_STEPS)
    return step_keywords("gcode"), step_keywords("svg")
