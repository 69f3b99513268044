"""The component sort keys of stage 08-B (k_comp_keys: a thread per skeleton pixel) on the cases of tests/comp_key_cases.py: components of 1, 63, 64, 65
and 8 381 pixels, a smallest block key late in raster order, equal block indices in two groups.  Stage 08 against the oracle under the same parameter
block, lines with their order and taps, equality; each case also with ORIP_COMP_CAPS forcing the larger component classes.  The order of the output
seldom depends on a key's exact value (a component's first pixel and its smallest block lie in the same row of blocks), so the keys themselves are read
through ORIP_COMP_DBG and held against a numpy restatement on the oracle's skeleton: per group the sorted block keys, as a multiset over the groups.
tests/test_oracle_comp_key_cases.py shows on the CPU that the cases hold these components."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import comp_key_cases as K
import skel_path_cases as C
from util import same_polys, cfgobj

_want = {}


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def blocks(W, H, over):
    """(the ABI struct, the oracle's parameter block) with the overrides in both, as tests/test_gpu_skel_path_cases.py builds them"""
    from orip import stages as S
    cfgd = dict(O.DEFAULTS, **C.CFG)
    prm = S.params08(cfgobj(cfgd))
    names = [n for n, _ in prm._fields_]
    want = dict(zip(names, O.derived08(cfgd))); want.update(W=W, H=H); want.update(over)
    prm.W = W; prm.H = H
    for k, v in over.items():
        setattr(prm, k, v)
    return prm, np.array([want[n] for n in names], np.float64)


@pytest.mark.parametrize("caps", [None, K.CAPS], ids=["default_classes", "forced_classes"])
@pytest.mark.parametrize("name,W,H,polys,over", K.CASES, ids=[c[0] for c in K.CASES])
def test_stage08b_component_keys(dev, monkeypatch, name, W, H, polys, over, caps):
    from orip import lib as L
    monkeypatch.delenv("ORIP_HASH_SORT", raising=False)
    if caps is None:
        monkeypatch.delenv("ORIP_COMP_CAPS", raising=False)
    else:
        monkeypatch.setenv("ORIP_COMP_CAPS", caps)
    prm, want_prm = blocks(W, H, over)
    if name not in _want:
        _want[name] = O.stage08_layer(polys, want_prm)
    want_l, want_t = _want[name]
    dev.set_polys(L.SLOT_SORTED, 0, polys)
    dev.dedup_layer(0, prm)
    assert dev.get_taps(L.TAPS_INTRA, 0) == want_t
    got_l = dev.get_polys(L.SLOT_LINES_INTRA, 0)
    assert same_polys(got_l, want_l), (len(got_l), len(want_l))


def oracle_keys(name):
    """per group the sorted smallest block keys of its components, by tests/test_oracle_skel_path_cases.py's restatement of k_comp_keys"""
    import test_oracle_comp_key_cases as TK
    import test_oracle_skel_path_cases as T
    groups, _ = TK.groups_of(name)
    return sorted(tuple(sorted(int(k) for k in T.comp_keys(g))) for g in groups if g["comps"])


@pytest.mark.parametrize("name,W,H,polys,over", K.CASES, ids=[c[0] for c in K.CASES])
def test_component_keys_are_the_minimum_over_the_component(dev, monkeypatch, capfd, name, W, H, polys, over):
    from orip import lib as L
    monkeypatch.delenv("ORIP_COMP_CAPS", raising=False)
    monkeypatch.setenv("ORIP_COMP_DBG", "1")
    prm, _ = blocks(W, H, over)
    dev.set_polys(L.SLOT_SORTED, 0, polys)
    capfd.readouterr()
    dev.dedup_layer(0, prm)
    err = capfd.readouterr().err
    by_rank = {}
    for line in err.splitlines():
        if line.startswith("[comp dbg] rank "):
            w = line.split()
            by_rank.setdefault(int(w[3]), []).append(int(w[5]))
    got = sorted(tuple(sorted(v)) for v in by_rank.values())
    assert got == oracle_keys(name)
