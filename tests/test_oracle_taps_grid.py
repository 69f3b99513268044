"""The cases of taps_grid_cases.py on the CPU: every case through the oracle's stage10_layer, the plain restatement of the sequential rule (verdicts) agreeing
with it, and from the verdicts the proof that every case holds what its name claims: how many candidates are accepted, which one refuses which, how deep the
chain of decisions is that the kernel's rounds have to follow."""
import numpy as np
import pytest

from oracle import oracle as O
import cross_cases as X
import taps_grid_cases as T

CASES = T.cases()
_V = {}


def cands_of(c):
    return c["layers"][0][1]


def oracle_taps(c):
    forb = np.zeros((c["H"], c["W"]), np.uint8)
    lines, taps = O.stage10_layer(c["layers"][0][0], cands_of(c), forb, X.prm_vec(X.prm_of(c)))
    return taps


def verdicts(name):
    if name not in _V:
        c = CASES[name]
        _V[name] = T.verdicts(cands_of(c), T.forb_of(c), T.radius_of(c))
    return _V[name]


def states(name):
    return [s for s, _ in verdicts(name)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_rule_is_the_oracle(name):
    c = CASES[name]
    want = [p for p, (s, _) in zip(cands_of(c), verdicts(name)) if s == T.ACC]
    assert oracle_taps(c) == want
    assert 64 <= c["W"] <= 256 and 64 <= c["H"] <= 256 and T.radius_of(c) in T.RADII
    assert T.lds_bytes(len(cands_of(c))) <= T.LDS_LIMIT          # the one-workgroup kernel takes it


@pytest.mark.parametrize("r", T.RADII)
def test_counts_and_kinds(r):
    for n in T.COUNTS:
        name = "count_%d_r%d" % (n, r)
        assert len(cands_of(CASES[name])) == n
    v = verdicts("count_129_r%d" % r)
    why = [w for _, w in v]
    assert "off" in why and "free" in why and any(isinstance(w, int) for w in why)      # off the canvas, accepted inside, refused by an earlier one
    if r == 70:
        inside = [p for p, (s, w) in zip(cands_of(CASES["count_129_r70"]), v) if w != "off"]
        assert len({T.cell(p, r) for p in inside}) == 1                                 # a cell wider than the canvas


@pytest.mark.parametrize("r", T.RADII)
def test_boundary(r):
    vs = T.ON_CIRCLE[r] + [T.JUST_OUTSIDE[r]]
    assert all(a * a + b * b == r * r for a, b in T.ON_CIRCLE[r]) and T.JUST_OUTSIDE[r][0] ** 2 + T.JUST_OUTSIDE[r][1] ** 2 == r * r + 1
    if r == 70:
        got = [states("boundary_r70_%d" % i) for i in range(len(vs))]
    else:
        s = states("boundary_r%d" % r)
        got = [s[2 * i:2 * i + 2] for i in range(len(vs))]
    assert got == [[T.ACC, T.OUT]] * len(T.ON_CIRCLE[r]) + [[T.ACC, T.ACC]]


@pytest.mark.parametrize("r", T.RADII)
def test_chains(r):
    at_r, beyond = "chain_r%d_step%d" % (r, r), "chain_r%d_step%d" % (r, r + 1)
    n = len(cands_of(CASES[at_r]))
    assert n == {1: 200, 3: 86, 70: 4}[r]
    assert states(at_r) == [T.ACC, T.OUT] * (n // 2)                                      # alternating
    assert [w for _, w in verdicts(at_r)][1::2] == list(range(0, n, 2))                   # each refused by the one before it
    assert T.depth(cands_of(CASES[at_r]), T.forb_of(CASES[at_r]), r) == n                 # as many rounds as candidates
    m = len(cands_of(CASES[beyond]))
    assert m == {1: 128, 3: 64, 70: 4}[r] and states(beyond) == [T.ACC] * m
    if r == 1:
        assert states("chain_r1_diag") == [T.ACC] * 200


@pytest.mark.parametrize("r", T.RADII)
def test_repeated_and_full_cell(r):
    assert states("repeated_r%d" % r) == [T.ACC] + [T.OUT] * 99
    c = CASES["full_cell_r%d" % r]
    assert len({T.cell(p, r) for p in cands_of(c)}) == 1 and len(cands_of(c)) == 80
    s = states("full_cell_r%d" % r)
    assert s.count(T.ACC) >= 1 and s.count(T.OUT) >= 40


@pytest.mark.parametrize("r", T.RADII)
def test_borders(r):
    c = CASES["borders_r%d" % r]
    W, H = c["W"], c["H"]
    cells = {T.cell(p, r) for p in cands_of(c)}
    for corner in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
        assert T.cell(corner, r) in cells
    assert any(x % r == 0 and x > 0 for x, _ in cands_of(c)) and any(x % r == r - 1 for x, _ in cands_of(c))
    v = verdicts("borders_r%d" % r)
    refused_across = [(i, w) for i, (s, w) in enumerate(v) if isinstance(w, int) and T.cell(cands_of(c)[i], r) != T.cell(cands_of(c)[w], r)]
    assert refused_across or r == 1          # a candidate refused by one in a neighbouring cell (at r = 1 a cell is one pixel: every refusal but a duplicate's is)
    assert states("borders_r%d" % r).count(T.ACC) >= 4


@pytest.mark.parametrize("r", T.RADII)
def test_off_canvas_and_raster(r):
    c = CASES["off_canvas_r%d" % r]
    v = verdicts("off_canvas_r%d" % r)
    off = [i for i, (_, w) in enumerate(v) if w == "off"]
    assert len(off) == 8 and any(cands_of(c)[i][0] < 0 for i in off) and any(cands_of(c)[i][0] >= c["W"] for i in off) and any(cands_of(c)[i][1] >= c["H"] for i in off)
    assert sum(1 for _, w in v if isinstance(w, int) and w in off) >= 3                  # inside candidates refused by one off the canvas
    assert cands_of(c)[0] == cands_of(c)[1] and v[0][0] == v[1][0] == T.ACC              # the same point twice off the canvas: both stay
    assert [w for _, w in verdicts("raster_r%d" % r)] == ["free", "raster", "free", "free", "raster", 3]


def test_empty_and_lds():
    assert cands_of(CASES["empty"]) == [] and oracle_taps(CASES["empty"]) == []
    assert T.lds_bytes(T.LDS_N["lds_over"]) > T.LDS_LIMIT >= T.lds_bytes(T.LDS_N["lds_under"]) and T.LDS_N["lds_over"] == T.LDS_N["lds_under"] + 1
