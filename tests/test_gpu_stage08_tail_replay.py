"""The sequential tail replay of stage 08-A as the product runs it: k_tail_par marks a polyline with its last unsure sample and k_tail_replay redoes it
up to there, in windows of 64 operations, with the plain loop for a sample of more than 63 pops.  Every case of tests/tail_replay_cases.py compares
S.dedup_layer with the oracle's stage08_layer, lines and taps, bit-exact, in the style of tests/test_gpu_stage08_chain.py (snakes whose rows lie closer
than the collision radius: nearly every pop count shows in the result).  tests/test_oracle_tail_replay_cases.py shows on the CPU that each case holds
the unsure samples, the sure stretch and the pop count it is built for."""
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import tail_replay_cases as C
from util import cfgobj, same_polys

SEQ = "ORIP_TAIL_SEQ"
_want = {}


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def want_of(name, polys, cfgd):
    if name not in _want:
        _want[name] = O.stage08_layer(polys, O.derived08(cfgd))
    return _want[name]


RUNS = [(c[0], False) for c in C.CASES] + [(n, True) for n in sorted(C.SEQ_TOO)]


@pytest.mark.parametrize("name, seq", RUNS, ids=[n + ("-seq" if s else "") for n, s in RUNS])
def test_stage08_tail_replay(dev, monkeypatch, name, seq):
    from orip import stages as S
    _, over, polys, _ = next(c for c in C.CASES if c[0] == name)
    if seq:
        monkeypatch.setenv(SEQ, "1")
    else:
        monkeypatch.delenv(SEQ, raising=False)          # the replay as the product path: only what k_tail_par marks, up to the mark
    monkeypatch.delenv("ORIP_TAIL_DBG", raising=False)
    cfgd = dict(O.DEFAULTS, **over)
    want_l, want_t = want_of(name, polys, cfgd)
    got_l, got_t = S.dedup_layer(polys, cfgobj(cfgd), dev)
    assert got_t == want_t
    assert same_polys(got_l, want_l), (len(got_l), len(want_l))
    assert len(want_l) + len(want_t) > 0
