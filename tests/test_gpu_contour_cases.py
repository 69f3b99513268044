"""Stage 04 on the structured skeletons of tests/contour_cases.py, against the oracle: the skeleton bytes and the contour lists with their order,
equality throughout.  These maps run what only the device compiles (walker.h: Wave::run, the LDS window and its three row loaders, chain_jump;
raster04.hip: k_chain_ends_bits, k_chain_build, the sizing of the chain lists, the thinning loop and its cap); tests/test_oracle_contour_cases.py
proves on the CPU that they have the chain lengths, placements and sizes that reach those paths, and the [walk dbg] counters checked below show
that the device did take them.  Every family runs under the switches that must change nothing."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
from util import same_polys
import contour_cases as C

# must change no result: the chain lists off; step and state logs of one entry per skeleton pixel (room_left is then bounded by the log room and
# the overflow retry of trace_finish runs on these shapes); every trace launched from orip_contours_layer instead of orip_contours_prepare
SWITCHES = {"default": {}, "no_chains": {"ORIP_NO_CHAINS": "1"}, "log_f1": {"ORIP_TRACE_LOG_F": "1"}, "trace_late": {"ORIP_TRACE_LATE": "1"}}

DBG = re.compile(r"\[walk dbg\] layer (\d+) NC=\d+ M=\d+ F=(\d+): .*?\| largest fg=(\d+): w1=(\d+) s1=\d+ w2=(\d+) s2=\d+ hit=\d+ det=\d+ tiles=(\d+) jumped=(\d+) calls=(\d+) rounds=(\d+)")


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


_want = {}


def want(name, build=None):
    """(names, stack, oracle skeletons, oracle contours, longest listed chain of the largest component) of a family, computed once and left unchanged"""
    if name not in _want:
        names, st = (build or C.FAMILIES[name])()
        sks = [O.thin_rot(e) for e in st]
        longest = []
        for sk in sks:
            n, lab = O.ccl8(sk)
            sizes = np.bincount(lab.ravel(), minlength=n)[1:]
            big = (lab == 1 + int(np.argmax(sizes))) if len(sizes) else np.zeros_like(lab, bool)
            longest.append(max(C.listed_lengths(np.where(big, sk, 0)), default=0))
        polys = [[p for p in O.trace(sk) if len(p) >= 5] for sk in sks]          # O.stage04 of the map, its thinning done once
        _want[name] = (names, st, sks, polys, longest)
    return _want[name]


def run_and_compare(dev, name, st, sks, polys, late=False):
    from orip.lib import SLOT_CONTOURS
    dev.set_edges(st)
    if late:
        dev.contours_prepare()
    else:
        dev.find_contours()
    for l in range(st.shape[0]):
        if late:
            dev.contours_layer(l)
        assert np.array_equal(dev.get_skeleton(l), sks[l]), (name, l, "skeleton")
        got = dev.get_polys(SLOT_CONTOURS, l)
        assert same_polys(got, polys[l]), (name, l, "contours", len(got), len(polys[l]))


def walk_counters(err):
    """{layer: dict of the largest component's counters} from the [walk dbg] lines"""
    out = {}
    for m in DBG.finditer(err):
        l, F, fg, w1, w2, tiles, jumped, calls, rounds = (int(v) for v in m.groups())
        out[l] = dict(F=F, fg=fg, walks=w1 + w2, tiles=tiles, jumped=jumped, calls=calls, rounds=rounds)
    return out


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name", list(C.FAMILIES))
def test_family_equals_oracle(dev, monkeypatch, capfd, name, switch):
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("ORIP_WALK_DBG", "1")
    names, st, sks, polys, longest = want(name)
    capfd.readouterr()
    run_and_compare(dev, (name, switch), st, sks, polys, late=switch == "trace_late")
    dbg = walk_counters(capfd.readouterr().err)
    assert sorted(dbg) == list(range(len(names))), (name, switch, sorted(dbg))
    for l, n in enumerate(names):
        d = dbg[l]
        print(f"{name}/{n} [{switch}] longest listed chain of the largest component {longest[l]}: {d}")
        # ---- that the paths ran
        if switch == "no_chains":
            assert d["jumped"] == 0 and d["calls"] == 0, (name, n, d)
        if name in C.CLOSED:
            # one component without endpoints: every pixel is visited by leftover walks, so a listed chain (>= 24 with an end) is met at an end pixel
            # with all of it but that pixel ahead -- at least 23 >= 8 forced steps; nothing shorter and no ring is listed, so nothing may be jumped
            if longest[l] == 0:
                assert d["jumped"] == 0 and d["rounds"] == 0, (name, n, d)
            elif switch in ("default", "trace_late"):
                assert d["jumped"] > 0 and d["calls"] > 0, (name, n, d)
                if longest[l] >= 89:
                    assert d["rounds"] >= 2, (name, n, d)              # a round takes at most 64 pixels
        if name == "open" and n in C.LONG_OPEN:
            assert d["tiles"] > d["walks"], (name, n, d)               # the window was re-placed along the way, not only loaded once per walk
    if switch == "log_f1" and name == "loops":
        # F = 1: a component's step log holds fg + 256 codes, while the own steps of its leftover walks pass the chains of these loops in both
        # directions before they meet a recorded trajectory (up to 2 * fg and more): for the loops of 500 .. 1300 pixels that cannot fit, so
        # trace_finish must have traced some layer again with 4x the logs
        assert max(d["F"] for d in dbg.values()) > 1, dbg


def test_chain_lists_too_small_then_sized_from_the_map_itself():
    """The chain lists are sized from the skeleton of the context's previous prepare (contour_cases.cap_ends_after / cap_cpix_after): after `small`,
    `crowded` has more than twice the chain ends and twice the chain pixels that fit, so most of its chains are not listed and are stepped through;
    run again, the lists are sized from `crowded` itself and everything fits.  Every run equals the oracle."""
    from orip.device import Device
    small = want("capacity_small", C.capacity_small)
    crowded = want("capacity_crowded", C.capacity_crowded)
    d = Device(0)
    try:
        for tag, (names, st, sks, polys, _) in (("small", small), ("crowded after small", crowded), ("crowded again", crowded), ("small again", small)):
            run_and_compare(d, tag, st, sks, polys)
    finally:
        d.close()
