"""Stage 12 (orip_plot_order, csrc/vector.hip) on the device at its edges: the cases of plot_order_cases.py through set_polys / set_taps / plot_order against the
oracle's raw op rows (type, line index, flip, x, y), by equality.  Every case runs under both kernels: as the library chooses (k_plot_order_wave while the lists
fit its LDS), and with ORIP_PLOT_1WG set, which the library reads at every call (k_plot_order, 1024 threads).  The two cases at the LDS limit run with no switch:
there the list sizes alone choose the kernel.  tests/test_oracle_plot_order_cases.py shows on the CPU what every case reaches and pins the hand-worked answers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import plot_order_cases as C

SMALL = C.small_cases()
KERNELS = [False, True]
KERNEL_IDS = ["as_chosen", "one_workgroup"]
_WANT = {}


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def want(name, case):
    if name not in _WANT:
        _WANT[name] = O.ops12_raw(*case)
    return _WANT[name]


def run(dev, lines, taps, R, layer=0):
    from orip import lib as L
    dev.set_polys(L.SLOT_LINES_CROSS, layer, lines); dev.set_taps(L.TAPS_CROSS, layer, taps)
    return dev.plot_order(layer, R)


def _kernel(monkeypatch, one_workgroup):
    if one_workgroup:
        monkeypatch.setenv("ORIP_PLOT_1WG", "1")
    else:
        monkeypatch.delenv("ORIP_PLOT_1WG", raising=False)


@pytest.mark.parametrize("one_workgroup", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("name", sorted(SMALL))
def test_case_rows(dev, monkeypatch, name, one_workgroup):
    _kernel(monkeypatch, one_workgroup)
    got = run(dev, *SMALL[name])
    w = want(name, SMALL[name])
    assert got.dtype == np.int32 and got.shape == w.shape, (got.shape, w.shape)
    assert np.array_equal(got, w), np.nonzero((got != w).any(1))[0][:5]


@pytest.mark.parametrize("one_workgroup", KERNELS, ids=KERNEL_IDS)
def test_answers_worked_by_hand(dev, monkeypatch, one_workgroup):
    """the device against the literals themselves"""
    _kernel(monkeypatch, one_workgroup)
    for name, (lines, taps, R, lit) in C.HAND.items():
        assert [tuple(int(v) for v in r) for r in run(dev, lines, taps, R)] == lit, name


@pytest.mark.parametrize("name", sorted(C.LDS_CASES))
def test_lds_limit_chooses_the_kernel(dev, monkeypatch, name):
    """8800 lines with 438 taps are 6 bytes past the wave kernel's LDS and take k_plot_order; with 437 taps they fit by 3 bytes"""
    _kernel(monkeypatch, False)
    case = C.lds_case(name)
    assert np.array_equal(run(dev, *case), want(name, case))


@pytest.mark.parametrize("one_workgroup", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("name", sorted(C.REFUSED))
def test_refusal_beyond_2p24(dev, monkeypatch, name, one_workgroup):
    """one coordinate one past +-2^24 is refused with an error that names the limit; the context goes on working"""
    from orip.device import OripError
    _kernel(monkeypatch, one_workgroup)
    lines, taps = C.REFUSED[name]
    with pytest.raises(OripError, match=r"16777216 \(2\^24\)"):
        run(dev, lines, taps, C.R0)
    good = SMALL["wide_pm_2p24"]                             # the contract's own corners, right after the refusal
    assert np.array_equal(run(dev, *good), want("wide_pm_2p24", good))
