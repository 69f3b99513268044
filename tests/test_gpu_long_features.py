"""The perimeters of long polylines (more than ORIP_LONG_POLY = 192 points: one block each, numpy's pairwise tree from leaf sums) to the last bit.
No ABI returns PolyFeat::per, so the tests use what the perimeter decides: stage 08-A draws the kept polylines longest first.

1. Explicit lists through S.dedup_layer (ESrc, leaves from the points, forward sum): the pairs of tests/long_feature_cases.py -- one float32 ulp apart,
   the other way round under a left-to-right sum, overlapping, so that the lines depend on the rank (tests/test_oracle_long_features.py) -- at 193, 194,
   257, 2049, 2181 and 4300 points, in both input orders.  All six sizes were found.
2. The resident chain from an image (VSrc, stage 07's prefetch, leaves from stored segment lengths, both reading directions), and again with
   ORIP_NO_PREFETCH08 (leaves from the points of the walk records).  The chain takes no chosen point lists: the image holds filled rectangles whose
   contours have open views of 194, 195, 274, 2066, 2090, 2242 and 4354 points; every artefact of the chain is compared with the oracle's."""
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import long_feature_cases as C
from util import cfgobj, same_polys, compare_resident, compare_ops


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("first", ["shorter", "longer"])
@pytest.mark.parametrize("n", C.SIZES)
def test_stage08_rank_of_one_ulp_pairs(dev, n, first):
    from orip import stages as S
    lo, hi = C.pair(n)
    polys = [lo, hi] if first == "shorter" else [hi, lo]
    want_l, want_t = O.stage08_layer(polys, O.derived08(C.CFG6))
    got_l, got_t = S.dedup_layer(polys, cfgobj(C.CFG6), dev)
    assert got_t == want_t
    assert same_polys(got_l, want_l), (len(got_l), len(want_l))


@pytest.fixture(scope="module")
def chain_want():
    return O.run_pipeline(C.chain_image(), C.chain_cfg())


@pytest.mark.parametrize("prefetch", [True, False])
def test_resident_chain_long_contours(dev, monkeypatch, chain_want, prefetch):
    from orip import stages as S
    if prefetch:
        monkeypatch.delenv("ORIP_NO_PREFETCH08", raising=False)
    else:
        monkeypatch.setenv("ORIP_NO_PREFETCH08", "1")
    cfgd = C.chain_cfg()
    ops = S.run_path(C.chain_image(), cfgobj(cfgd), dev)
    compare_resident(dev, cfgd, chain_want)
    compare_ops(ops, chain_want["ops"], cfgd["color_names"])
