"""Stage 04's memo planes are never cleared as a whole (walker.h: WalkArgs::memo): the launch of a layer's trace zeroes the eight words of every skeleton
pixel of that layer and nothing else, so whatever an earlier step left anywhere else must never be read.  One Device, one step after another, each step
compared with the oracle (skeletons and contour lists, equality) exactly as tests/test_gpu_contour_cases.py does.  The maps are closed shapes of
tests/contour_cases.py (figure eights, nested rings, a ring of degree-2 pixels): without an endpoint every pixel is reached by leftover walks, the
walks that fill and read the memo.  The order of the steps puts stale words at, next to and far from the live ones (memo_reuse_cases below), and
tests/test_memo_reuse_host.py shows on the CPU that this very sequence gives other contours when the live words are NOT cleared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import contour_cases as C
from memo_reuse_cases import sequence
from test_gpu_contour_cases import run_and_compare, want as family_want

_want = {}


def want(tag, st):
    """(oracle skeletons, oracle contours) of a stack, computed once and left unchanged"""
    if tag not in _want:
        sks = [O.thin_rot(e) for e in st]
        _want[tag] = (sks, [[p for p in O.trace(sk) if len(p) >= 5] for sk in sks])
    return _want[tag]


def step(dev, tag, st, reserve, late=False):
    """one step as the resident chain does it: image, the reserve hint (K as given; None: no hint), then stage 04 on the edge maps"""
    K, H, W = st.shape
    sks, polys = want(tag, st)
    if reserve is not None:
        dev.set_image(np.zeros((H, W, 3), np.uint8))
        dev.contours_reserve(reserve(K))
    run_and_compare(dev, tag, st, sks, polys, late=late)


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


# the hint with the right K, with a wrong one (one plane only / more planes than layers), and no hint: it clears nothing, so nothing may depend on it
RESERVE = {"right_k": lambda K: K, "wrong_k": lambda K: 1 if K > 1 else 3, "no_reserve": None}


@pytest.mark.parametrize("mode", list(RESERVE))
def test_sequence_equals_oracle_whatever_the_reserve(dev, monkeypatch, mode):
    for v in ("ORIP_TRACE_LATE", "ORIP_TRACE_LOG_F", "ORIP_NO_CHAINS", "ORIP_WALK_DBG"):
        monkeypatch.delenv(v, raising=False)
    for tag, st in sequence():
        step(dev, tag, st, RESERVE[mode])


def test_sequence_through_prepare_and_layer(dev, monkeypatch):
    """ORIP_TRACE_LATE's path: orip_contours_prepare enqueues no trace, every orip_contours_layer launches its own"""
    monkeypatch.delenv("ORIP_TRACE_LOG_F", raising=False)
    monkeypatch.setenv("ORIP_TRACE_LATE", "1")
    for tag, st in sequence():
        step(dev, tag, st, RESERVE["right_k"], late=True)


def test_overflow_retry_is_a_second_launch_after_one_prepare(dev, monkeypatch):
    """ORIP_TRACE_LOG_F=1 on `loops`: the logs of its larger loops overflow (tests/test_gpu_contour_cases.py asserts that they do), trace_finish traces
    the layer again with larger logs -- the second launch after one prepare, over the memo words and visited bits the overflowed trace left.  Twice,
    with a step of the sequence in between: the second run finds the planes as `loops` and that step left them."""
    monkeypatch.delenv("ORIP_TRACE_LATE", raising=False)
    monkeypatch.setenv("ORIP_TRACE_LOG_F", "1")
    names, st, sks, polys, _ = family_want("loops")
    tag0, st0 = sequence()[0]
    for _ in range(2):
        run_and_compare(dev, "loops", st, sks, polys)
        step(dev, tag0, st0, RESERVE["no_reserve"])
