"""GPU parity of stage 08-B on the deterministic cases of tests/skel_merge_cases.py: near-parallel lines whose stamped bands and skeletons lie on the
word, tile-column and tile-row boundaries of the bit-plane kernels (pack, tiled thinning, run-based CCL with the linear pixel id, compaction, heads), at
padded widths that are a multiple of 64, one more and one less.  Expected values come from the oracle under the same parameter block;
tests/test_oracle_skel_merge_cases.py shows on the CPU that 08-B merges something on every case.  Everything is equality: point lists with their order, taps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import skel_merge_cases as C
from util import same_polys, cfgobj


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("name,W,H,polys", C.cases(), ids=[c[0] for c in C.cases()])
def test_stage08b_on_word_and_tile_boundaries(dev, monkeypatch, name, W, H, polys):
    from orip import lib as L, stages as S
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    monkeypatch.delenv("ORIP_COMP_CAPS", raising=False)
    cfgd = dict(O.DEFAULTS, **C.CFG)
    prm = S.params08(cfgobj(cfgd))
    names = [n for n, _ in prm._fields_]
    want_prm = C.params(dict(zip(names, O.derived08(cfgd))), W, H)
    prm.W = W; prm.H = H
    want_l, want_t = O.stage08_layer(polys, np.array([want_prm[n] for n in names], np.float64))
    assert len(want_l) >= 1
    dev.set_polys(L.SLOT_SORTED, 0, polys)
    dev.dedup_layer(0, prm)
    assert dev.get_taps(L.TAPS_INTRA, 0) == want_t
    got_l = dev.get_polys(L.SLOT_LINES_INTRA, 0)
    assert same_polys(got_l, want_l), (len(got_l), len(want_l))
