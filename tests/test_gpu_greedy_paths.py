"""Stage 07's greedy order on every path of vreorder: the grid kernel, the brute-force kernel over its LDS store and over its global-memory store
(256 and 1024 threads), each at the list sizes and coordinate ranges that select it.  S.sort_contours against O.sort07, bit-exact.  The inputs are
those of tests/greedy_cases.py; tests/test_oracle_greedy_paths.py shows on the CPU which kernel each of them selects and that ties and closed
contours occur along the order."""
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import greedy_cases as C
from util import same_polys


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def expected():
    """the oracle's order of every case, computed once (the 16 001 polylines take seconds)"""
    return {name: O.sort07(C.polys_of(name)) for name in C.CASES}


@pytest.mark.parametrize("name", list(C.CASES))
def test_stage07_every_greedy_kernel(dev, monkeypatch, expected, name):
    from orip import stages as S
    if C.CASES[name][5]:
        monkeypatch.setenv("ORIP_NN_NOGRID", "1")
    else:
        monkeypatch.delenv("ORIP_NN_NOGRID", raising=False)
    assert same_polys(S.sort_contours(C.polys_of(name), dev), expected[name])
