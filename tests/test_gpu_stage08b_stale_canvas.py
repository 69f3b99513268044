"""Stage 08-B on a canvas it never clears (vector08b.hip, B08::gid): the calls of tests/stale_canvas_cases.py follow one another on ONE Device, so every
call finds the canvas, the bit planes and every scratch slot as the call before left them, and every call must equal the oracle (lines with their order,
taps) as tests/test_gpu_skel_merge_cases.py asserts it for a fresh canvas.  tests/test_oracle_stale_canvas_cases.py shows on the CPU that the stale stamps
lie where a reader that strayed off this call's stamped pixels would meet them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import skel_merge_cases as C
import stale_canvas_cases as SC
from util import same_polys, cfgobj

_want = {}


def want(W, brush):
    """[(name, W, H, polylines, oracle lines, oracle taps)] of a sequence, computed once and left unchanged"""
    if (W, brush) not in _want:
        from orip import stages as S
        cfgd = dict(O.DEFAULTS, **SC.CFG)
        names = [n for n, _ in S.params08(cfgobj(cfgd))._fields_]
        base = dict(zip(names, O.derived08(cfgd)))
        out = []
        for name, w, h, polys in SC.sequence(W, brush):
            d = C.params(base, w, h, post_brush=brush)
            wl, wt = O.stage08_layer(polys, np.array([d[n] for n in names], np.float64))
            out.append((name, w, h, polys, wl, wt))
        _want[(W, brush)] = out
    return _want[(W, brush)]


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("brush", SC.BRUSHES)
@pytest.mark.parametrize("W", SC.WIDTHS)
def test_calls_in_sequence_equal_the_oracle(dev, monkeypatch, W, brush):
    from orip import lib as L, stages as S
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    monkeypatch.delenv("ORIP_COMP_CAPS", raising=False)
    for name, w, h, polys, want_l, want_t in want(W, brush):
        prm = S.params08(cfgobj(dict(O.DEFAULTS, **SC.CFG)))
        prm.W = w; prm.H = h; prm.post_brush = brush
        dev.set_polys(L.SLOT_SORTED, 0, polys)
        dev.dedup_layer(0, prm)
        assert dev.get_taps(L.TAPS_INTRA, 0) == want_t, (name, W, brush)
        got_l = dev.get_polys(L.SLOT_LINES_INTRA, 0)
        assert same_polys(got_l, want_l), (name, W, brush, len(got_l), len(want_l))
