"""The stroke passes in combination, on the CPU: the rows of tests/compose_cases.py cover what they claim, the two drawings give every pass work whenever
its option is on, and the streams of the all-double runs have the consequences that need no double at all -- read off the decoded bytes (the decoder of
tests/stream_preview_double.py), so they also hold the host glue that the double run and the device run share (stroke_stream, _cut_result, the sources
behind dash and link, the pens of the dots), which equality between those two runs cannot see.  tests/test_gpu_compose.py then holds the device to these
same all-double runs, byte for byte."""
import itertools
import time

import numpy as np
import pytest

import compose_cases as CC
import stream_preview_double as SPD

DOORS = ("svg", "gcode")
ROW_SECONDS = 2.0                       # no all-double run of a row may take longer: a condition on the drawings
_RUNS = {}


def key_of(row):
    return tuple(sorted(row.items()))


def run(door, row):
    """(bytes, info, seconds, plot) of a row through the doubles, once"""
    k = (door, key_of(row))
    if k not in _RUNS:
        t = time.perf_counter()
        data, info = CC.run_doubles(door, row)
        _RUNS[k] = (data, info, time.perf_counter() - t, plot(data))
    return _RUNS[k]


def label(door, row):
    return " ".join(CC.words(door, row)[len(CC.BASE[door]):]) or "(nothing on)"


# ------------------------------------------------------------------ the decoded stream
def plot(data):
    """what the bytes draw, from the decoder alone: per pen colour the sorted keys of the undirected lattice steps made with the pen down, the taps as
    (x, y, colour), the pen-up steps, the pen-down steps, the pen-down segments"""
    st, kind, val = SPD.decode(data)
    isstep = kind == SPD.K_STEP
    d = np.where(isstep, val, 0)
    dx, dy = np.where(isstep, SPD.DX[d], 0), np.where(isstep, SPD.DY[d], 0)
    x, y = np.cumsum(dx), np.cumsum(dy)
    pen = kind == SPD.K_PEN
    down_after = SPD._ffill(pen, (val == 2).astype(np.int64), 0)
    down = np.concatenate([[0], down_after[:-1]]) if len(kind) else down_after
    colour = SPD._ffill(kind == SPD.K_COLOR, val, -1)
    assert st["eof_seen"] == 1 and st["unknown_service_bytes"] == 0 and (len(x) == 0 or (x.min() >= 0 and y.min() >= 0 and x.max() < 4096 and y.max() < 4096))
    ink = np.flatnonzero(isstep & (down == 1))
    a, b = (x[ink] - dx[ink]) * 4096 + (y[ink] - dy[ink]), x[ink] * 4096 + y[ink]
    keys = (np.minimum(a, b) << 24) | np.maximum(a, b)
    assert (colour[ink] >= 0).all()
    inked = {int(c): np.unique(keys[colour[ink] == c]) for c in np.unique(colour[ink])}
    points = {int(c): np.unique(np.concatenate([a[colour[ink] == c], b[colour[ink] == c]])) for c in np.unique(colour[ink])}
    tp = np.flatnonzero(pen & (val == 3))
    taps = sorted(zip(x[tp].tolist(), y[tp].tolist(), colour[tp].tolist()))
    return dict(inked=inked, points=points, ink_points=np.stack([x[ink], y[ink], x[ink] - dx[ink], y[ink] - dy[ink]], 1), taps=taps, travel=int((isstep & (down == 0)).sum()), down_steps=len(ink),
                segments=int((pen & (val == 2) & (down == 0)).sum()), steps=st["steps_total"], bytes=st["total_bytes"])


def same_ink(p, q, exact=True):
    """the two plots ink the same undirected lattice steps with every pen.  exact=False, for a pair of runs of which one may draw strokes backwards
    (--allow-reverse): the stream compiler walks a segment from its first point and, where the exact line passes midway between two lattice points, takes the
    nearer-to-the-start one (tests/stream_double.py: codes_numpy, ceil((2 k d - D) / (2 D)) is round-half-down of k d / D), so a segment drawn backwards takes the
    other point there: the two step sets differ by such points alone.  Then every inked point of either plot has an inked point of the same pen of the other
    within one lattice step, and the pens are the same; a stroke lost, moved, doubled onto another pen or drawn elsewhere is farther off than that"""
    if p["inked"].keys() != q["inked"].keys():
        return False
    if exact:
        return all(np.array_equal(p["inked"][c], q["inked"][c]) for c in p["inked"])
    for c in p["inked"]:
        for u, v in ((p["points"][c], q["points"][c]), (q["points"][c], p["points"][c])):
            near = np.unique(np.concatenate([v + 4096 * i + j for i, j in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))]))      # the minor coordinate moves by one, the major stays
            if not np.isin(u, near).all():
                return False
    return True


# ------------------------------------------------------------------ coverage
@pytest.mark.parametrize("door", DOORS)
def test_rows_cover_what_they_claim(door):
    rows, F = CC.rows(door), CC.FACTORS[door]
    assert len(rows) == CC.ROW_COUNTS[door] <= CC.MAX_ROWS and rows == CC.generate_rows(door)    # deterministic
    assert all(set(r) == set(F) and all(0 <= r[n] < len(F[n]) for n in F) and CC.allowed(door, r) for r in rows)
    assert rows[0] == {n: 0 for n in F} and rows[1] == CC.ALL_ON[door] and len({tuple(sorted(r.items())) for r in rows}) == len(rows)
    assert all(r[n] for r in rows[1:2] for n in F)
    pairs = triples = 0
    for names in itertools.combinations(F, 2):
        for lv in itertools.product(*(range(len(F[n])) for n in names)):
            if CC.allowed(door, dict(zip(names, lv))):
                pairs += 1
                assert any(all(r[n] == v for n, v in zip(names, lv)) for r in rows), (names, lv)
    for names in itertools.combinations(CC.REWRITING[door], 3):
        for lv in itertools.product(*(range(len(F[n])) for n in names)):
            if CC.allowed(door, dict(zip(names, lv))):
                triples += 1
                assert any(all(r[n] == v for n, v in zip(names, lv)) for r in rows), (names, lv)
    assert pairs > 100 and triples > 100


@pytest.mark.parametrize("door", DOORS)
def test_every_refused_combination_raises_and_nothing_else_is_excluded(door):
    F = CC.FACTORS[door]
    for extra in CC.REFUSED[door]:
        with pytest.raises(ValueError):
            CC.run_doubles(door, extra)
    refused = 0
    for names in itertools.combinations(F, 2):                                                    # what the predicate excludes, the door refuses: in the smallest row that holds it
        for lv in itertools.product(*(range(len(F[n])) for n in names)):
            if not CC.allowed(door, dict(zip(names, lv))):
                refused += 1
                with pytest.raises(ValueError):
                    CC.run_doubles(door, dict({n: 0 for n in F}, **dict(zip(names, lv))))
    assert refused == (2 if door == "svg" else 1)                                                 # --no-reorder --improve-order; --hatch-connect without a hatch
    # every full combination of levels the predicate allows parses: the rows are a sample of these, and none of them is refused (the work test runs the rows)
    assert all(CC.allowed(door, dict(zip(F, lv))) == (not (lv[list(F).index("order")] == CC.NO_REORDER and lv[list(F).index("improve")]) and
                                                      not (door == "svg" and lv[list(F).index("connect")] and not lv[list(F).index("hatch")]))
               for lv in itertools.product(*(range(len(F[n])) for n in F)))


# ------------------------------------------------------------------ work
def work_failures(door, row, info):
    """the counters that say a pass that is on did nothing, by name; the exceptions are stated here, each with its reason"""
    on = lambda n: row.get(n, 0) > 0
    bad = []

    def need(name, ok):
        if not ok:
            bad.append(name)
    if on("clip"):
        need("clip.cut", info["clip"]["cut"] > 0)
    if on("dash"):
        need("dash.dashes > dash.dashed > 0", info["dash"]["dashes"] > info["dash"]["dashed"] > 0)
    if on("connect"):
        # EXCEPTED: hatch level 5, --no-serpentine.  Every line then runs left to right, so a link is the diagonal back across the shape, and the narrowest hatched
        # stretch of the drawing (the U's legs, 46 mm) is wider than the reach (16 mm): nothing is in reach, as the README says of the combination
        need("hatch_link.links", info["hatch_link"]["links"] > 0 or row["hatch"] == 5)
    if on("occlude"):
        need("occlude.cut", info["occlude"]["cut"] > 0); need("occlude.hidden", info["occlude"]["hidden"] > 0)
    if on("dedup"):
        need("dedup.covered + dedup.cut", info["dedup"]["covered"] + info["dedup"]["cut"] > 0)
    if on("merge"):
        need("merge.joins", info["merge"]["joins"] > 0)
    if on("simplify"):
        need("simplify.points_out < points_in", info["simplify"]["points_out"] < info["simplify"]["points_in"])
    if on("stipple"):
        need("stipple.dots", info["stipple"]["dots"] > 0 and info["taps"] == info["stipple"]["dots"])
        if on("occlude"):
            need("stipple.hidden", info["stipple"]["hidden"] > 0)
    if on("reverse"):
        # EXCEPTED: --no-reorder.  File order was asked for, and _order then reverses nothing
        need("pens.reversed", (info["pens"] if on("pens") else info)["reversed"] > 0 or row["order"] == CC.NO_REORDER)
    return bad


@pytest.mark.parametrize("door", DOORS)
def test_every_pass_that_is_on_has_work_in_every_row(door):
    rows = CC.rows(door)
    bad, some = [], {k: set() for k in ("eligible", "cycles", "seam", "improve", "ring")}
    slowest, most = (0.0, None), 0
    for row in rows:
        data, info, sec, _ = run(door, row)
        slowest = max(slowest, (sec, label(door, row)))
        most = max(most, info["paths"] + info.get("taps", 0))
        names = work_failures(door, row, info)
        if names:
            bad.append((label(door, row), names))
        if "hatch_link" in info and info["hatch_link"]["eligible"] < info["hatch_link"]["in_reach"]: some["eligible"].add(0)
        if "merge" in info and info["merge"]["cycles"] > 0: some["cycles"].add(0)
        if "seam" in info and info["seam"]["moved"] > 0: some["seam"].add(0)
        if "improve" in info and info["improve"]["travel_after"] < info["improve"]["travel_before"]: some["improve"].add(0)
        if "ring_entry" in info and info["ring_entry"]["moved"] > 0: some["ring"].add(row["pens"])
    print(f"{door}: {len(rows)} rows, at most {most} strokes and dots, slowest all-double row {slowest[0]:.2f} s: {slowest[1]}")
    assert most <= CC.MAX_OPS
    assert not bad, "\n".join(f"{l}: {n}" for l, n in bad)
    assert some["cycles"] and some["seam"] and some["improve"] and some["ring"] == {0, 1, 2} and (some["eligible"] or door == "gcode")
    assert slowest[0] <= ROW_SECONDS, slowest


# ------------------------------------------------------------------ consequences on the bytes
def inside_strictly(poly, x, y):
    """even-odd, in integers; a point on an edge is not inside"""
    n, odd = len(poly), False
    for (ax, ay), (bx, by) in zip(poly, poly[1:] + poly[:1]):
        cr = (bx - ax) * (y - ay) - (by - ay) * (x - ax)
        if cr == 0 and min(ax, bx) <= x <= max(ax, bx) and min(ay, by) <= y <= max(ay, by):
            return False
        if (ay > y) != (by > y) and ((cr > 0) == (by > ay)):
            odd = not odd
    return odd


def svg_shapes_in_steps(info, invert_y):
    """the filled shapes of the SVG drawing in steps, in paint order, as the conversion places them: page mm = (x, 297 - y), times the steps per mm, y turned
    round under --invert-y.  Under the clamp a shape that leaves the sheet is clamped point by point, as its outline is"""
    W, H = info["target"]
    out = []
    for name, poly in CC.SVG_FILLED:
        q = [(x * CC.SVG_STEPS_PER_MM, int(round((CC.SVG_HEIGHT_MM - y) * CC.SVG_STEPS_PER_MM))) for x, y in poly]
        q = [(x, H - 1 - y if invert_y else y) for x, y in q]
        if "clip" not in info:
            q = [(min(max(x, 0), W - 1), min(max(y, 0), H - 1)) for x, y in q]
        out.append((name, q))
    return out


def consequence_failures(door, row):
    data, info, _, p = run(door, row)
    bad = []

    def need(name, ok):
        if not ok:
            bad.append(name)
    # 6. the counts of info are those of the bytes
    need("info paths/taps/steps/bytes", (info["paths"], info.get("taps", 0), info["steps"], info["bytes"]) == (p["segments"], len(p["taps"]), p["steps"], len(data)) and p["bytes"] == len(data))
    need("steps = pen-down + pen-up", p["steps"] == p["down_steps"] + p["travel"])
    # 5. the pen-up travel of the bytes is what the last reporting pass states
    last = info["seam"]["travel_after"] if "seam" in info else info["improve"]["travel_after"] if "improve" in info else info["ring_entry"]["travel"] if "ring_entry" in info else None
    if last is not None:
        need("pen-up travel", p["travel"] == last)
    if "seam" in info and "improve" in info:
        need("seam.travel_before == improve.travel_after", info["seam"]["travel_before"] == info["improve"]["travel_after"])
    if "improve" in info and "ring_entry" in info:
        need("improve.travel_before == ring_entry.travel", info["improve"]["travel_before"] == info["ring_entry"]["travel"])
    # 4. nothing outside the clip rectangle; no tap in a shape painted later
    if row["clip"]:
        x0, y0, x1, y1 = info["clip"]["rect"]
        q = p["ink_points"]
        need("ink inside the clip rectangle", len(q) == 0 or ((q[:, [0, 2]] >= x0).all() and (q[:, [0, 2]] <= x1).all() and (q[:, [1, 3]] >= y0).all() and (q[:, [1, 3]] <= y1).all()))
        need("taps inside the clip rectangle", all(x0 <= x <= x1 and y0 <= y <= y1 for x, y, _ in p["taps"]))
    if door == "svg" and row["stipple"]:
        shapes = svg_shapes_in_steps(info, row["invert_y"])
        own = [[k for k, (_, poly) in enumerate(shapes) if inside_strictly(poly, x, y)] for x, y, _ in p["taps"]]
        need("every tap lies in a filled shape", all(own))
        at = [t[:2] for t in p["taps"]]
        if row["occlude"]:
            # one lattice for the whole drawing: where shapes overlap each has a candidate on the same point, and all but the topmost shape's are hidden.  So no point
            # is tapped twice, and (the pens on) a tap has the colour of the topmost shape that holds it: the dot of a shape painted earlier would show another
            need("no tap under a shape painted later: a point tapped twice", len(set(at)) == len(at))
            if row["pens"]:
                need("no tap under a shape painted later: the colour is not the topmost shape's", all(c == CC.SVG_FILL_PEN[k[-1]] for k, (_, _, c) in zip(own, p["taps"])))
        else:
            need("without --occlude the shapes that overlap tap a point once each", len(set(at)) < len(at))
    # 1. the options that only reorder leave the ink of every pen and the taps as they are.  Lattice step for lattice step where no run of the pair may draw a
    # stroke backwards; same_ink states what holds where one may.  --allow-reverse also lets the merge join strokes against their direction, which is no
    # reordering: with --merge-paths the sibling keeps it
    plain = CC.reorder_off(row)
    if row["merge"] and row["reverse"]:
        plain = dict(plain, reverse=1)
    exact = not row["reverse"]
    if plain != row:
        q = run(door, plain)[3]
        need("reorder-only options change the ink", same_ink(p, q, exact)); need("reorder-only options change the taps", p["taps"] == q["taps"])
        need("reorder-only options change the pen-down steps or the strokes", (p["down_steps"], p["segments"]) == (q["down_steps"], q["segments"]))
    # 2, 3. merge, simplify 0 and dedup leave the inked set; dedup never adds a pen-down step.  Compared where no tolerance is on: behind --simplify-mm 0.1 other
    # strokes are other polylines
    base = dict(row, simplify=min(row["simplify"], 1))
    b = run(door, base)[3]
    if row["merge"]:
        q = run(door, dict(base, merge=0))[3]
        need("--merge-paths changes the ink", same_ink(b, q, exact)); need("--merge-paths changes the pen-down steps", b["down_steps"] == q["down_steps"])
    if base["simplify"] == 1:
        q = run(door, dict(base, simplify=0))[3]
        need("--simplify-mm 0 changes the ink", same_ink(b, q, exact)); need("--simplify-mm 0 changes the pen-down steps", b["down_steps"] == q["down_steps"])
    if row["dedup"]:
        q = run(door, dict(base, dedup=0))[3]
        need("--dedup changes the inked set", same_ink(b, q, exact)); need("--dedup adds pen-down steps", b["down_steps"] <= q["down_steps"])
    return bad


@pytest.mark.parametrize("door", DOORS)
def test_consequences_on_the_decoded_bytes(door):
    bad = []
    for row in CC.rows(door):
        names = consequence_failures(door, row)
        if names:
            bad.append((label(door, row), names))
    assert not bad, "\n".join(f"{l}: {n}" for l, n in bad)
