"""k_chain_build steps on the degree-2 bit plane (raster04.hip): figures whose chains cross the words of that plane and touch the image's sides, against
the oracle with the chain lists and with ORIP_NO_CHAINS=1 (per-pixel stepping: the same contours).  K = 2, the second layer the mirror image of the
first, so that what touches x = 0 also touches x = W - 1 and every crossing is taken in both directions (each end of a chain walks it; the smaller owns
it).  The [walk dbg] line shows that the lists were used: in a figure without end points every pixel is reached by leftover walks, so a listed chain
(an end, at least 24 pixels) must be jumped, and where nothing can be listed nothing may be."""
import re

import numpy as np
import pytest

from oracle import oracle as O
from util import same_polys
import contour_cases as C

DBG = re.compile(r"\[walk dbg\] layer (\d+) NC=\d+ M=\d+ F=\d+: .*?\| largest fg=\d+: w1=\d+ s1=\d+ w2=\d+ s2=\d+ hit=\d+ det=\d+ tiles=\d+ jumped=(\d+) calls=(\d+) rounds=\d+")
R = 20                                           # diamond of 41 x 41: arcs of 37 (halves) and 35 (chord) degree-2 pixels, all listed
S = 2 * R + 1


def _canvas(H, W, items):
    e = np.zeros((H, W), np.uint8)
    for shape, y0, x0 in items:
        C._put(e, shape, y0, x0)
    return e


def figures():
    """name -> (plane, closed): closed = no end point anywhere, so the jumped counter is decided by what is listed"""
    th, ring = C.diamond(R), C.diamond(R, chord=False)
    out = {}
    for W in (63, 64, 65, 130):
        # flush with x = W - 1, y = 0 and y = H - 1 (mirrored: x = 0).  W = 130: a second theta whose apexes lie at x = 64, so its chord crosses x = 63 | 64
        # horizontally and its left-hand diagonals cross it going down-right and up-right (walked from the other end: up-left, down-left).  The ring's
        # side corner is a degree-2 pixel at x = W - 1: at W = 65 and 130 its two diagonals cross 63 | 64 and 127 | 128.  (No chain can cross into the
        # last column horizontally: its pixel there would need a second neighbour that also touches the pixel before it.)
        items = [(th, 0, W - S)] + ([(th, 0, 44)] if W == 130 else [])
        out[f"theta_W{W}"] = (_canvas(S, W, items), True)
        out[f"ring_W{W}"] = (_canvas(S, W, [(ring, 0, W - S)]), True)
        # arcs of exactly 23 (not listed), 24 and 25 degree-2 pixels: up to x = W - 1, at W = 130 horizontally across x = 63 | 64 instead
        for n in (23, 24, 25):
            out[f"arc{n}_W{W}"] = (_canvas(C.THETA_H + 4, W, [(C.theta(n), 2, 50 if W == 130 else W - (25 + 4) - (25 - n))]), True)
    z = np.zeros((48, 2), np.uint8)
    z[np.arange(48), np.arange(48) & 1] = 255                       # the two-column zigzag: one open chain of 46 degree-2 pixels, diagonal steps only
    out["zigzag_W2"] = (z, False)
    return out


_want = {}


def want(name):
    if name not in _want:
        e, closed = figures()[name]
        e = O.thin_rot(e)                                            # (the chord's ends lose their corner pixels: the figure IS its skeleton from here on)
        st = np.stack([e, e[:, ::-1]])
        sks = [O.thin_rot(x) for x in st]
        polys = [[p for p in O.trace(sk) if len(p) >= 5] for sk in sks]
        listed = [C.listed_lengths(sk) for sk in sks]
        ends = [bool((C.degrees(sk) == 1).any()) for sk in sks]
        _want[name] = (st, sks, polys, listed, ends, closed)
    return _want[name]


NAMES = list(figures())


# ---------------------------------------------------------------- no GPU: the figures are what the docstring says
@pytest.mark.parametrize("name", NAMES)
def test_figures_have_the_chains_they_are_named_for(name):
    st, sks, polys, listed, ends, closed = want(name)
    assert st.shape[1] <= 48 and st.shape[2] in (2, 63, 64, 65, 130)
    for l in range(2):
        assert np.array_equal(sks[l], st[l]), (name, l, "already one pixel wide")
        assert ends[l] == (not closed), (name, l)
        assert len(polys[l]) >= 1, (name, l)
        if name.startswith("theta"):
            assert listed[l] == sorted([2 * R - 3, 2 * R - 3, 2 * R - 5] * (2 if name.endswith("W130") else 1)), (name, listed[l])
        elif name.startswith("ring"):
            assert listed[l] == [] and (C.degrees(sks[l])[sks[l] > 0] == 2).all(), (name, listed[l])
        elif name.startswith("arc"):
            n = int(name[3:5])
            assert listed[l] == ([n] * 3 if n >= C.CHAIN_MIN else []), (name, listed[l])
            assert sorted(len(p) for p, e in C.chains(sks[l]) if e)[-3:] == [n] * 3, name
        else:
            assert listed[l] == [46], (name, listed[l])
    d2 = C.degrees(sks[0]) == 2
    hor = lambda b: bool((d2[:, b] & d2[:, b + 1]).any())
    down_right = lambda b: bool((d2[:-1, b] & d2[1:, b + 1]).any())         # walked from its other end: up-left
    up_right = lambda b: bool((d2[1:, b] & d2[:-1, b + 1]).any())
    if name == "theta_W130":
        assert hor(63) and down_right(63) and up_right(63), name
    if name in ("ring_W65", "ring_W130"):
        b = 63 if name == "ring_W65" else 127                       # the ring's side corner lies at x = W - 1 = 64 or 129, its diagonals come in across b | b + 1
        assert down_right(b) and up_right(b), name
    if name.startswith("arc") and name.endswith("W130"):
        assert hor(63), name


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["default", "no_chains"])
@pytest.mark.parametrize("name", NAMES)
def test_contours_equal_oracle_and_lists_are_used(dev, monkeypatch, capfd, name, switch):
    from orip.lib import SLOT_CONTOURS
    if switch == "no_chains":
        monkeypatch.setenv("ORIP_NO_CHAINS", "1")
    monkeypatch.setenv("ORIP_WALK_DBG", "1")
    st, sks, polys, listed, ends, closed = want(name)
    capfd.readouterr()
    dev.set_edges(st)
    dev.find_contours()
    for l in range(2):
        assert np.array_equal(dev.get_skeleton(l), sks[l]), (name, l, "skeleton")
        got = dev.get_polys(SLOT_CONTOURS, l)
        assert same_polys(got, polys[l]), (name, switch, l, len(got), len(polys[l]))
    dbg = {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in DBG.finditer(capfd.readouterr().err)}
    assert sorted(dbg) == [0, 1], (name, switch, dbg)
    for l in range(2):
        jumped, calls = dbg[l]
        print(f"{name} [{switch}] layer {l}: listed {listed[l]}, jumped {jumped}, calls {calls}")
        if switch == "no_chains" or (closed and not listed[l]):
            assert jumped == 0, (name, switch, l, dbg[l])
        elif closed:
            assert jumped > 0 and calls > 0, (name, switch, l, dbg[l])
