"""The stroke passes in combination, on the GPU: every row of tests/compose_cases.py, through both vector front doors with no step given, against the same row
through the doubles alone -- the bytes, and every key of info -- without a tolerance anywhere.  On the device every pass from the dedup on reads what the
pass before it left resident and not the arrays the host holds, so a disagreement between the two shows only here.  One Device for the module: the rows run
forward and then backward on it, and the two doors take turns on it, so a pass that reads a leftover of the drawing before out of a buffer that only grows
gives other bytes in one of the two positions.  tests/test_compose_host.py says what the rows cover and what the all-double runs are worth."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import compose_cases as CC

BATCH = 8
_WANT, _FORWARD = {}, {}


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def key_of(door, row, want_paths=False):
    return door, tuple(sorted(row.items())), want_paths


def want(door, row, want_paths=False):
    """the all-double run of a row, computed once and left unchanged"""
    k = key_of(door, row, want_paths)
    if k not in _WANT:
        _WANT[k] = CC.run_doubles(door, row, want_paths)
    return _WANT[k]


def with_paths(door, i):
    """fitted_paths are compared on the all-off and the all-on row of the SVG door (the G-code door has none)"""
    return door == "svg" and i < 2


def check(dev, door, row, want_paths=False):
    """"" or the report of a mismatch; the device's bytes"""
    exp, winfo = want(door, row, want_paths)
    got, info = CC.run_device(door, row, dev, want_paths)
    assert "timings" not in info and "timings" not in winfo
    return CC.mismatch(door, row, got, info, exp, winfo), got


def batches():
    """per door: the rows forward, eight to an item, then the same rows backward"""
    out = []
    for door in ("svg", "gcode"):
        n = len(CC.rows(door))
        idx = list(range(n))
        for way, seq in (("forward", idx), ("backward", idx[::-1])):
            out += [pytest.param(door, way, seq[a:a + BATCH], id=f"{door}-{way}-{a // BATCH}") for a in range(0, n, BATCH)]
    return out


@pytest.mark.parametrize("door,way,idx", batches())
def test_every_row_on_the_device_is_the_all_double_run(dev, door, way, idx):
    rows = CC.rows(door)
    bad = []
    for i in idx:
        msg, got = check(dev, door, rows[i], with_paths(door, i))
        if msg:
            bad.append(msg)
        if way == "forward":
            _FORWARD[(door, i)] = got
        elif (door, i) in _FORWARD and got != _FORWARD[(door, i)]:                                # the same row behind a larger and behind a smaller drawing
            bad.append(f"{door}: {' '.join(CC.words(door, rows[i]))}\n  the bytes differ between the forward and the backward pass over the rows: something is carried over")
    assert not bad, "\n".join(bad)


def test_the_two_doors_take_turns_on_one_device(dev):
    """the SVG door leaves fitted paths resident and the G-code door does not use them; ten rows of each, interleaved"""
    bad = []
    for i in range(2, 12):
        for door in ("svg", "gcode"):
            msg, _ = check(dev, door, CC.rows(door)[i])
            if msg:
                bad.append(msg)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("door", ["svg", "gcode"])
def test_given_and_own_passes_mixed(dev, door):
    """a given pass in front of one of the device's own: the device is sent the strokes where the host alone holds them and reads its resident list where
    the pass before was its own (tests/test_stroke_residency_host.py holds the forms; here the device's kernels take them).  The all-on row under every
    assignment of recording_device.assignments, five further rows under the two that alternate"""
    import recording_device as RD
    rows, text, bad = CC.rows(door), CC.SVG_TEXT if door == "svg" else CC.GCODE_TEXT, []
    for i in (1, 2, 3, 4, 5, 6):
        row, o = rows[i], CC.options(door, rows[i])
        exp, winfo = want(door, row)
        for given in RD.assignments(RD.factors_on(door, row))[slice(None) if i == 1 else slice(1, 3)]:
            got, info = RD.run_mixed(door, o, text, given, dev, door == "svg" and o.hatch_angle_deg is not None and o.hatch_spacing_mm is not None)
            msg = CC.mismatch(door, row, got, info, exp, winfo)
            if msg:
                bad.append("given: " + " ".join(n for n in given if given[n]) + "\n" + msg)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("door", ["svg", "gcode"])
def test_all_on_row_on_a_device_of_its_own(door):
    """nothing can be carried over here: a failure is the row's own"""
    from orip.device import Device
    d = Device(0)
    try:
        row = CC.rows(door)[1]
        assert row == CC.ALL_ON[door]
        msg, got = check(d, door, row, with_paths(door, 1))
    finally:
        d.close()
    assert not msg, msg
    exp, winfo = want(door, row, with_paths(door, 1))
    assert got == exp and all(k in winfo for k in ("clip", "pens", "dash", "dedup", "merge", "simplify", "ring_entry", "improve", "seam"))
    if door == "svg":
        assert all(k in winfo for k in ("hatch", "hatch_u", "hatch_link", "occlude", "stipple", "taps", "fitted_paths")) and isinstance(winfo["fitted_paths"][1], np.ndarray)
