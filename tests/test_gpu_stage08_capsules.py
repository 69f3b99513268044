"""Stage 08-A4, the capsule table behind the set in LDS (k_caps_insert): a workgroup owns a range of R samples, keeps the capsule keys it has seen with the
smallest sample index of each, and sends to the table only the first occurrence of a key in its range and what the set had no room for.  The table must
still end up with the smallest index per capsule over the whole layer.  Every case compares S.dedup_layer with the oracle's stage08_layer, lines and taps,
bit-exact, on the 1 260 x 1 782 canvas; the sample counts the cases are built for come from the oracle's own resampling and are asserted before the GPU
runs.  The inputs are capsule_cases.py's: rings walked lap after lap so that lap 3 repeats the capsules of lap 1 exactly and lap 2 is dropped by nothing but
the sample indices lap 1's capsules carry (test_oracle_capsule_cases.py shows that without a GPU).

The host picks R from the layer's sample count, and a layer of a few thousand samples gets R = 1 024; ORIP_CAPS_RANGE forces a range, so that the same
input meets a set that filters inside one chunk, over later chunks of a range, and over several ranges.  ORIP_CAPSSET_TINY leaves the set 32 slots (nearly
every sample finds no room and goes to the table as before), ORIP_CAPS_TINY starts the table at 1 024 slots (the growth rounds: every round starts the
sets from empty)."""
import pytest

pytestmark = pytest.mark.gpu

import capsule_cases as C
from util import cfgobj, same_polys

RANGES = [None, "8192", "16384", "65536"]
HOOKS = ("ORIP_CAPS_RANGE", "ORIP_CAPSSET_TINY", "ORIP_CAPS_TINY")


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def check(dev, monkeypatch, name, rng=None, hook=None):
    from orip import stages as S
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    if rng:
        monkeypatch.setenv("ORIP_CAPS_RANGE", rng)
    if hook:
        monkeypatch.setenv(hook, "1")
    polys = C.CASES[name]
    assert [len(s) for s in C.samples(name)] == [C.n_samples(p) for p in polys]
    want_l, want_t = C.expected(name)
    got_l, got_t = S.dedup_layer(polys, cfgobj(C.CFG), dev)
    assert got_t == want_t
    assert same_polys(got_l, want_l), (len(got_l), len(want_l))


# ---------------------------------------------------------------- shapes 1 - 3: repeats in the chunk, in a later chunk, beyond the largest range
@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("name", ["ring400_3laps", "ring1400_3laps", "ring1400_50laps"])
def test_capsules_laps(dev, monkeypatch, name, rng):
    check(dev, monkeypatch, name, rng)


# ---------------------------------------------------------------- shape 4: the ring starts anywhere in a chunk and in a range
@pytest.mark.parametrize("rng", [None, "8192"])
@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_capsules_ring_behind_lead_chunk(dev, monkeypatch, n, rng):
    """the ring's first sample (ORIP_PXY_FIRST) is sample 1023 of chunk 0, sample 0 and sample 1 of chunk 1"""
    check(dev, monkeypatch, "lead%d_ring300" % n, rng)


@pytest.mark.parametrize("R", [8192, 16384])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_capsules_ring_behind_lead_range(dev, monkeypatch, R, d):
    """the ring starts at the last sample of a range, at the first and at the second of the next one"""
    check(dev, monkeypatch, "lead%d_ring400" % (R + d), str(R))


# ---------------------------------------------------------------- shape 5: repeats across polylines and ranges
@pytest.mark.parametrize("rng", [None, "2048", "8192"])
def test_capsules_two_polylines_one_ring(dev, monkeypatch, rng):
    check(dev, monkeypatch, "two_over_one_ring", rng)


# ---------------------------------------------------------------- shape 6: k_caps_insert<true>
@pytest.mark.parametrize("rng", [None, "8192"])
def test_capsules_ring_leaves_canvas(dev, monkeypatch, rng):
    check(dev, monkeypatch, "ring_leaves_canvas", rng)


# ---------------------------------------------------------------- shapes 7, 8: 1 - 3 again with a set of 32 slots, and with the table's growth rounds
@pytest.mark.parametrize("hook", ["ORIP_CAPSSET_TINY", "ORIP_CAPS_TINY"])
@pytest.mark.parametrize("rng", [None, "8192", "65536"])
@pytest.mark.parametrize("name", ["ring400_3laps", "ring1400_3laps", "ring1400_50laps"])
def test_capsules_laps_hooks(dev, monkeypatch, name, rng, hook):
    check(dev, monkeypatch, name, rng, hook)
