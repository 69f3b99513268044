"""The pairs of tests/long_feature_cases.py are what tests/test_gpu_long_features.py needs them to be, shown with the oracle alone: one float32 ulp
between the two perimeters, the opposite order under a left-to-right float32 sum, and another stage-08 result when the two swap ranks.  CPU only."""
import numpy as np
import pytest

from oracle import oracle as O
import long_feature_cases as C
from util import same_polys


@pytest.mark.parametrize("n", C.SIZES)
def test_pair_properties(n):
    found = C.pair(n)
    assert found is not None, "no pair among the candidates"
    lo, hi = found
    assert len(lo) == len(hi) == n and not (lo[0] == lo[-1]).all() and not (hi[0] == hi[-1]).all()       # open, n points
    p_lo, p_hi = np.float32(O.poly_perimeter(lo)), np.float32(O.poly_perimeter(hi))
    assert p_hi == np.nextafter(p_lo, np.float32(np.inf))                                                  # exactly one ulp
    for p, per in ((lo, p_lo), (hi, p_hi)):
        assert np.sum(C.seglen(p.reshape(-1, 2))) == per                                                   # numpy's own pairwise sum of these lengths
    assert C.sequential_sum(lo.reshape(-1, 2)) > C.sequential_sum(hi.reshape(-1, 2))                       # a plain sum ranks them the other way
    W, H = O.canvas_size(C.CFG6)
    for p in (lo, hi):
        a = p.reshape(-1, 2)
        assert a.min() >= 0 and a[:, 0].max() < W and a[:, 1].max() < H


@pytest.mark.parametrize("n", C.SIZES)
def test_stage08_depends_on_the_rank(n):
    lo, hi = C.pair(n)
    prm = O.derived08(C.CFG6)
    for polys, first in (([lo, hi], 1), ([hi, lo], 0)):                                                    # the longer one is drawn first wherever it stands
        want_l, want_t = O.stage08_layer(polys, prm)
        by_rank = C.stage08_in_rank(polys, [first, 1 - first])
        assert same_polys(by_rank[0], want_l) and by_rank[1] == want_t
        swapped = C.stage08_in_rank(polys, [1 - first, first])
        assert not same_polys(swapped[0], want_l)


def test_chain_image_has_contours_of_the_sizes():
    cfgd = C.chain_cfg()
    want = O.run_pipeline(C.chain_image(), cfgd)
    dark = cfgd["color_names"][0]
    sizes = C.open_view_sizes(want["sorted"][dark])
    assert C.CHAIN_SIZES <= set(sizes)
    assert any(192 < m <= 196 for m in sizes) and any(2048 < m <= 2048 + 132 for m in sizes) and any(2048 + 132 < m < 4096 for m in sizes) and any(m > 4096 for m in sizes)
    assert len(want["ops"][dark]) >= 10                      # (the layer leaves something to compare)


def test_sizes_straddle_the_limits():
    assert C.SIZES[:3] == [192 + 1, 192 + 2, 257] and C.SIZES[3:5] == [2048 + 1, 2048 + 132 + 1] and 2 * 2048 < C.SIZES[5] <= 3 * 2048
