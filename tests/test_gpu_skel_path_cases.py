"""GPU parity of stage 08-B on the cases of tests/skel_path_cases.py: every branch of the path choice and of the anchor rule, the component order, the
chunked FIFO search on junction-rich and fat skeletons, the three size classes and their boundaries, and post_brush, post_step, post_eps and post_minlen
away from their defaults, written into the ABI struct (no config key reaches them).  Expected values come from the oracle under the same parameter
block; tests/test_oracle_skel_path_cases.py shows on the CPU that every case reaches what its name says.  Everything is equality: point lists with
their order, taps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import skel_path_cases as C
from util import same_polys, cfgobj

CASES = C.cases()


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def _blocks(W, H, over):
    """(the ABI struct, the oracle's parameter block) with the overrides in both"""
    from orip import stages as S
    cfgd = dict(O.DEFAULTS, **C.CFG)
    prm = S.params08(cfgobj(cfgd))
    names = [n for n, _ in prm._fields_]
    want = dict(zip(names, O.derived08(cfgd))); want.update(W=W, H=H); want.update(over)
    prm.W = W; prm.H = H
    for k, v in over.items():
        setattr(prm, k, v)
    return prm, np.array([want[n] for n in names], np.float64)


def _check(dev, W, H, polys, over, what):
    from orip import lib as L
    prm, want_prm = _blocks(W, H, over)
    want_l, want_t = O.stage08_layer(polys, want_prm)
    dev.set_polys(L.SLOT_SORTED, 0, polys)
    dev.dedup_layer(0, prm)
    assert dev.get_taps(L.TAPS_INTRA, 0) == want_t, what
    got_l = dev.get_polys(L.SLOT_LINES_INTRA, 0)
    assert same_polys(got_l, want_l), (what, len(got_l), len(want_l))
    return want_l


@pytest.mark.parametrize("name,W,H,polys,over,caps", CASES, ids=[c[0] for c in CASES])
def test_stage08b_path_search_and_post_fields(dev, monkeypatch, name, W, H, polys, over, caps):
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    if caps is None:
        monkeypatch.delenv("ORIP_COMP_CAPS", raising=False)
    else:
        monkeypatch.setenv("ORIP_COMP_CAPS", caps)
    want_l = _check(dev, W, H, polys, over, name)
    assert len(want_l) >= 1 or name in ("minlen500", "minlen_path_plus1")


@pytest.mark.parametrize("over,message", C.REFUSALS, ids=[",".join(f"{k}={v}" for k, v in r[0].items()) for r in C.REFUSALS])
def test_stage08b_refusals_leave_the_lane_usable(dev, monkeypatch, over, message):
    from orip import lib as L
    from orip.device import OripError
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    monkeypatch.delenv("ORIP_COMP_CAPS", raising=False)
    prm, _ = _blocks(192, 192, over)
    dev.set_polys(L.SLOT_SORTED, 0, C.TIE)
    with pytest.raises(OripError, match=message):
        dev.dedup_layer(0, prm)
    assert len(_check(dev, 192, 192, C.TIE, {}, "default case after a refusal")) == 1
