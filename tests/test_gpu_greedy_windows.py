"""The grid kernel of the greedy order in its wide rounds (windows of 7 x 7 cells and more: one pass per 64 rows, the candidates 64 per trip across the
rows).  S.sort_contours against O.sort07, bit-exact, on the inputs of tests/greedy_window_cases.py, each twice: as it runs (the asm loop takes the common
steps and hands the others over at r = 3) and with ORIP_NN_NOASM=1 (every step through the compiled code, from r = 1).
tests/test_oracle_greedy_windows.py shows on the CPU which rounds, candidate counts, ties, closed contours and borders each input reaches."""
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import greedy_window_cases as W
from util import same_polys


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cases():
    """name -> (the polylines, the oracle's order), computed once"""
    out = {}
    for name, make in W.CASES.items():
        polys = make()
        out[name] = (polys, O.sort07(polys))
    return out


@pytest.mark.parametrize("no_asm", [False, True], ids=["asm", "noasm"])
@pytest.mark.parametrize("name", list(W.CASES))
def test_stage07_wide_rounds(dev, monkeypatch, cases, name, no_asm):
    from orip import stages as S
    monkeypatch.delenv("ORIP_NN_NOGRID", raising=False)
    if no_asm:
        monkeypatch.setenv("ORIP_NN_NOASM", "1")
    else:
        monkeypatch.delenv("ORIP_NN_NOASM", raising=False)
    polys, want = cases[name]
    assert same_polys(S.sort_contours(polys, dev), want)
