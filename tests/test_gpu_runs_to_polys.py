"""orip_runs_to_polys on the device (csrc/vector_common.hip): the flags of a layer's samples (stage 08-A) or of a line's cut steps (stage 10) -> polylines.
The inputs are those of runs_cases.py; test_oracle_runs_cases.py shows without a GPU what each of them selects, and every case here asserts the same
property again before it runs the device.  Stage 08 compares S.dedup_layer with the oracle's stage08_layer, stage 10 S.dedup_cross with O.stage10, lines
and taps, bit-exact.  The helper takes T slots per block and 16 per lane and load; the sample counts and the places of the accepted stretches are chosen
against those two numbers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
from util import cfgobj, same_polys

import runs_cases as R

T = 4096          # ORIP_RUN_TILE (csrc/vec_common.h); runs_cases.py builds its inputs on the same number
assert R.T == T


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("name", sorted(R.CASES08))
def test_stage08_runs(dev, monkeypatch, name):
    from orip import stages as S
    monkeypatch.delenv("ORIP_TAIL_SEQ", raising=False)
    R.holds08(name)
    polys, cfgd = R.CASES08[name][:2]
    want_l, want_t = O.stage08_layer(polys, O.derived08(cfgd))
    got_l, got_t = S.dedup_layer(polys, cfgobj(cfgd), dev)
    assert got_t == want_t
    assert same_polys(got_l, want_l), (len(got_l), len(want_l))


def test_stage08_empty_then_full_on_one_device(dev):
    """a layer with no accepted sample, one with every run a single, then a full one, on ONE lane: the early returns leave an empty list, and nothing of a
    call before shows in the next"""
    from orip import stages as S
    for name in ("all_accepted", "none_accepted", "two_polylines_on_tile_boundary", "every_run_single", "all_accepted"):
        R.holds08(name)
        polys, cfgd = R.CASES08[name][:2]
        want_l, want_t = O.stage08_layer(polys, O.derived08(cfgd))
        got_l, got_t = S.dedup_layer(polys, cfgobj(cfgd), dev)
        assert got_t == want_t and same_polys(got_l, want_l), name


@pytest.mark.parametrize("name", sorted(R.CASES10))
def test_stage10_runs(dev, name):
    from orip import stages as S
    R.holds10(name)
    intra = R.intra10(name)
    want = O.stage10(intra, R.CFG10)
    got = S.dedup_cross(intra, cfgobj(R.CFG10), dev)
    for n in R.CFG10["color_names"]:
        assert got[n][1] == want[n][1], n
        assert same_polys(got[n][0], want[n][0]), n
    if name == "all_allowed":
        assert len(want["layer_light"][0]) == 1 and len(want["layer_light"][0][0]) == R.L10 + 1
    if name in ("all_forbidden", "alternating_singles"):
        assert want["layer_light"] == ([], [])
