"""Stage 10's tap filter with its cell hash (k_taps_grid, csrc/vector10.hip) on the device: the cases of taps_grid_cases.py through set_polys / set_taps /
orip_dedup_cross / get_taps against the oracle's stage10_layer, by equality: the accepted taps and their order.  The library chooses the kernel; the two cases at
the LDS limit differ by one candidate, so that the size rule alone sends one to k_taps_grid and the other to k_taps_sequential.
tests/test_oracle_taps_grid.py shows on the CPU what every case reaches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import cross_cases as X
import taps_grid_cases as T

CASES = T.cases()


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def run(dev, c):
    from orip import lib as L
    lines, taps = c["layers"][0]
    dev.set_polys(L.SLOT_LINES_INTRA, 0, lines); dev.set_taps(L.TAPS_INTRA, 0, taps)
    p = X.prm_of(c)
    dev.dedup_cross([0], L.Params10(**{k: (int(p[k]) if k in ("tap_max_v", "W", "H") else float(p[k])) for k in X.FIELDS}))
    return dev.get_taps(L.TAPS_CROSS, 0)


def want(c):
    forb = np.zeros((c["H"], c["W"]), np.uint8)
    return O.stage10_layer(c["layers"][0][0], c["layers"][0][1], forb, X.prm_vec(X.prm_of(c)))[1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_case(dev, monkeypatch, name):
    monkeypatch.delenv("ORIP_TAPS_1WG", raising=False); monkeypatch.delenv("ORIP_PAINT_SEPARABLE", raising=False)
    assert run(dev, CASES[name]) == want(CASES[name])


@pytest.mark.parametrize("name", sorted(T.LDS_N))
def test_lds_limit_chooses_the_kernel(dev, monkeypatch, name):
    """9295 candidates are past the one-workgroup kernel's LDS and take k_taps_sequential by the size rule; 9294 fill k_taps_grid to its last 16 bytes"""
    monkeypatch.delenv("ORIP_TAPS_1WG", raising=False); monkeypatch.delenv("ORIP_PAINT_SEPARABLE", raising=False)
    c = T.lds_case(name)
    assert run(dev, c) == want(c)
