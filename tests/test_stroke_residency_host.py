"""The host driver of the vector front doors with some passes given and the others a device's own, on the CPU.  Every other test runs a door with every
step given (the doubles) or with none (the device); which passes read the polylines the pass before them left resident and which are sent their input is
decided between those two, and is held here.  The device is tests/recording_device.py: the doubles with a resident state of their own, so a resident read
of a list the stand-in does not hold, or holds in another state than the host, gives an error or other bytes, and every call is logged with its form.

Per door, per row of compose_cases, per assignment of recording_device.assignments over the factors the row switches on: the bytes and every key of info
are the all-double run's; the logged forms are what `predicted` below says -- the rule of DESIGN.md ("Stroke driver") and its exceptions, stated here
again, from the assignment alone --; and, over the whole set, every situation the rule tells apart has occurred.  The G-code rows do not flatten arcs, so
three rows with --arcs on a text with arcs are added for the flattening's two forms.  Written against the keywords of the doors alone."""
import numpy as np
import pytest

import compose_cases as CC
import recording_device as RD

DOORS = ("svg", "gcode")
ARC_TEXT = CC.GCODE_TEXT + "T0\nG0 X20 Y20\nM3\nG2 X40 Y40 I10 J10\nG3 X60 Y20 R20\nG1 X70 Y20\nM5\n"
ARC_ROWS = (0, 1, 5)                    # rows of the G-code door that are run once more with --arcs on ARC_TEXT
REWRITING = ("convert", "dash", "hatch_link", "occlude", "dedup", "merge", "simplify")
COMPARED = {"gcode_flatten", "gcode_to_steps", "gcode_to_steps_clip", "gcode_dash", "gcode_hatch_link", "svg_hatch_link", "gcode_occlude", "svg_occlude", "gcode_dedup",
            "gcode_merge", "gcode_simplify", "svg_stipple", "gcode_order", "gcode_order_pens", "gcode_order_rings", "gcode_improve", "gcode_seam"}
_SEEN = {}


def predicted(door, row, given, arcs=False):
    """(the calls of the device's own passes with their forms, in pipeline order; the situations this run is an instance of).  The rule: an own pass with a
    resident form reads the resident list iff the last pass that rewrote the stroke list was the device's own, else it is sent its input.  The exceptions:
    with the dots of a stipple among the strokes the ring order and the seam pass are always sent them; behind a ring order, which rotates the rings on the
    host, the seam pass is always sent them; an own occlusion or hatch link behind a given pass uploads the strokes through its ring-less form and then
    runs the form that reads the fitted paths; an own flattening leaves its paths resident only for an own conversion and is fetched for a given one.
    The orders and the improvement are sent the ends.  The SVG door's own conversion reads the fitted paths."""
    on = RD.factors_on(door, row, arcs)
    own = lambda name: name in on and not given[name]
    calls, tags = [], set()
    resident = False                    # the last pass that rewrote the stroke list was the device's own
    clip = "gcode_to_steps_clip" if row["clip"] else "gcode_to_steps"
    if own("flatten"):
        calls.append(("gcode_flatten", "uploaded"))
        tags.add("flatten left resident" if own("convert") else "flatten fetched")
        if not own("convert"):
            calls.append(("svg_paths", "resident"))
    if own("convert"):
        calls.append((clip, "resident" if door == "svg" or own("flatten") else "uploaded"))
    resident = own("convert")
    for name, method in (("dash", "gcode_dash"), ("hatch_link", "hatch_link"), ("occlude", "occlude"), ("dedup", "gcode_dedup"), ("merge", "gcode_merge"),
                         ("simplify", "gcode_simplify")):
        if name not in on:
            continue
        if own(name) and name in ("hatch_link", "occlude"):
            if not resident:
                calls.append(("gcode_" + method, "uploaded")); tags.add(name + " uploads first")
            else:
                tags.add(name + " reads resident")
            calls.append(("svg_" + method, "resident"))
        elif own(name):
            calls.append((method, "resident" if resident else "uploaded"))
        if own(name) and name in ("dash", "hatch_link"):
            tags.add(f"{name} own, sources {'given' if given['source'] else 'own'}")
        resident = own(name)
    stipple, ring = "stipple" in on, row["order"] == CC.RING_ENTRY
    if own("stipple"):
        calls.append(("svg_stipple", "resident"))
    if own("order"):
        if ring:
            calls.append(("gcode_order_rings", "resident" if resident and not stipple else "uploaded"))
            tags |= {"ring order sent the strokes with dots"} if resident and stipple else set()
        else:
            calls.append(("gcode_order_pens" if row["pens"] or row["reverse"] else "gcode_order", "uploaded"))
    if own("improve"):
        calls.append(("gcode_improve", "uploaded"))
    if own("seam"):
        calls.append(("gcode_seam", "resident" if resident and not stipple and not ring else "uploaded"))
        if resident and stipple:
            tags.add("seam sent the strokes with dots")
        elif resident and ring:
            tags.add("seam sent the strokes behind a ring order")
    return calls, tags


def cases(door):
    """(label, row, options, text, arcs) of every run of a door"""
    out = [(i, row, CC.options(door, row), CC.SVG_TEXT if door == "svg" else CC.GCODE_TEXT, False) for i, row in enumerate(CC.rows(door))]
    if door == "gcode":
        rows = CC.rows(door)
        out += [(f"arcs-{i}", rows[i], CC.options(door, CC.words(door, rows[i])[len(CC.BASE[door]):] + ["--arcs"]), ARC_TEXT, True) for i in ARC_ROWS]
    return out


def run_case(door, case):
    """every assignment of a case against the all-double run -> the list of failures; what was seen goes to _SEEN"""
    label, row, o, text, arcs = case
    if (door, label) in _SEEN:
        return _SEEN[(door, label)][0]
    names = RD.factors_on(door, row, arcs)
    angle = door == "svg" and o.hatch_angle_deg is not None and o.hatch_spacing_mm is not None
    if arcs:
        import arc_double as AD
        from orip import gcode as GC
        want, winfo = GC.build_stream_from_gcode(text, o, **dict(CC.gcode_doubles_all(), flatten_fn=AD.flatten_fn))
        assert "arcs" in winfo
    else:
        want, winfo = CC.run_doubles(door, row)
    bad, forms, tags = [], set(), set()
    for given in RD.assignments(names):
        dev = RD.RecordingDevice()
        what = f"{door} {label}: " + " ".join(("+" if given[n] else "-") + n for n in names)
        try:
            got, info = RD.run_mixed(door, o, text, given, dev, angle)
        except Exception as e:                                           # a resident read of what the stand-in does not hold
            bad.append(f"{what}\n  {type(e).__name__}: {e}")
            continue
        msg = CC.mismatch(door, row, got, info, want, winfo)
        if msg:
            bad.append(what + "\n  " + msg)
        calls, t = predicted(door, row, given, arcs)
        log = [c for c in dev.log if c[0] in COMPARED or (door == "gcode" and c[0] == "svg_paths")]
        if log != calls:
            bad.append(f"{what}\n  calls {log}\n  predicted {calls}")
        forms |= set(log); tags |= t
    _SEEN[(door, label)] = (bad, forms, tags)
    return bad


@pytest.mark.parametrize("door,k", [(door, k) for door in DOORS for k in range(len(CC.rows(door)) + (len(ARC_ROWS) if door == "gcode" else 0))])
def test_given_and_own_passes_mixed_give_the_all_double_run_in_the_predicted_forms(door, k):
    bad = run_case(door, cases(door)[k])
    assert not bad, "\n".join(bad)


def test_every_situation_of_the_residency_rule_occurs():
    forms, tags = set(), set()
    for door in DOORS:
        for case in cases(door):
            run_case(door, case)
            forms |= _SEEN[(door, case[0])][1]; tags |= _SEEN[(door, case[0])][2]
    both = ("gcode_to_steps", "gcode_to_steps_clip", "gcode_dash", "gcode_dedup", "gcode_merge", "gcode_simplify", "gcode_order_rings", "gcode_seam")
    missing = [(m, f) for m in both for f in ("resident", "uploaded") if (m, f) not in forms]
    assert not missing, missing
    want = {"flatten left resident", "flatten fetched", "hatch_link uploads first", "hatch_link reads resident", "occlude uploads first", "occlude reads resident",
            "ring order sent the strokes with dots", "seam sent the strokes with dots", "seam sent the strokes behind a ring order",
            "dash own, sources given", "dash own, sources own", "hatch_link own, sources given", "hatch_link own, sources own"}
    assert want <= tags, sorted(want - tags)
