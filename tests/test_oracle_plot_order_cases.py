"""The stage-12 cases of plot_order_cases.py on the CPU: every case through the oracle (its raw op rows are what test_gpu_plot_order_cases.py compares the
device with), the short answers stated by hand, and for every case the proof that it holds what its name claims -- read off the trace of the exact model in
plot_order_cases.py, which itself has to agree with the oracle row for row."""
import math

import numpy as np
import pytest

from oracle import oracle as O
import plot_order_cases as C

SMALL = C.small_cases()
_ROWS, _MODEL = {}, {}


def rows(name):
    if name not in _ROWS:
        _ROWS[name] = O.ops12_raw(*SMALL[name])
    return _ROWS[name]


def model(name):
    if name not in _MODEL:
        _MODEL[name] = C.model(*SMALL[name])
    return _MODEL[name]


def n_real(lines):
    return sum(1 for p in lines if np.asarray(p).reshape(-1, 2).shape[0] >= 2)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_model_is_the_oracle(name):
    """the model's rows are the oracle's rows, so its trace says what the oracle went through; every real line and every tap is an op exactly once"""
    lines, taps, R = SMALL[name]
    w = rows(name)
    assert w.dtype == np.int32 and w.shape == (n_real(lines) + len(taps), 5)
    assert np.array_equal(model(name)[0], w)
    assert sorted(int(k) for t, k, *_ in w if t == 0) == [i for i, p in enumerate(lines) if np.asarray(p).reshape(-1, 2).shape[0] >= 2]
    assert sorted((int(x), int(y)) for t, _, _, x, y in w if t == 1) == sorted(taps)
    # build_ops12 is the same rows as dicts
    ops = O.build_ops12(lines, taps, R)
    assert [o["type"] for o in ops] == ["line" if t == 0 else "tap" for t in w[:, 0]]


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_answers_worked_by_hand(name):
    assert [tuple(int(v) for v in r) for r in rows(name)] == C.HAND[name][3]


# ---------------------------------------------------------------- A.1
@pytest.mark.parametrize("n", C.TOTALS)
def test_totals(n):
    for kind in ("lines", "taps", "mixed"):
        name = "total_%d_%s" % (n, kind)
        if kind == "mixed" and n < 2:
            assert name not in SMALL
            continue
        lines, taps, _ = SMALL[name]
        assert len(lines) + len(taps) == n == len(rows(name))
        assert (len(lines) > 0, len(taps) > 0) == {"lines": (True, False), "taps": (False, True), "mixed": (True, True)}[kind]
    if n >= 64:
        # one pass of the drain emits the op that fills the 64-entry ring and, when the total allows, the op after it as well
        ev = [e for e in model("total_%d_mixed" % n)[1] if e["ev"] == "drain"]
        runs_at = {}
        for e in ev:
            runs_at.setdefault(e["nops"], e["run"])
        full = [m for m in range(64, n + 1, 64) if m - 1 in runs_at and (m == n or runs_at.get(m) == runs_at[m - 1])]
        assert full, sorted(runs_at)


# ---------------------------------------------------------------- A.2
@pytest.mark.parametrize("R", sorted(C.RADIUS_VECTORS))
def test_radius_taps_sit_on_the_radius(R):
    name = "radius_%g" % R
    lines, taps, r = SMALL[name]
    assert r == R
    drains = [e for e in model(name)[1] if e["ev"] == "drain"]
    picks = [e for e in model(name)[1] if e["ev"] == "pick"]
    for i, v in enumerate(C.RADIUS_VECTORS[R]):
        E = tuple(int(c) for c in lines[2 * i].reshape(-1, 2)[-1])
        q, p = taps[2 * i], taps[2 * i + 1]
        dq, dp = (q[0] - E[0]) ** 2 + (q[1] - E[1]) ** 2, (p[0] - E[0]) ** 2 + (p[1] - E[1]) ** 2
        assert (p[0] - E[0], p[1] - E[1]) == v
        if R == int(R):
            assert dp == int(R) ** 2 and dq > dp                     # exactly on the radius, and the neighbour just beyond
        else:
            assert dp == math.floor(R * R) and dq == dp + 1          # the last and the first whole d^2 on either side of R^2
        # P is drained from E itself; Q, although of lower index and alive, is not, and comes through the nearest search from P
        assert [e for e in drains if e["t"] == 2 * i + 1 and e["from"] == E and e["d2"] == dp]
        assert not [e for e in drains if e["t"] == 2 * i]
        assert [e for e in picks if e["idx"] == 2 * len(lines) + 2 * i]
    named = {80.0: [(80, 1)], 81.0: [(81, 1)], 80.5: [(80, 9)]}
    for v in named.get(R, []):
        assert any((q[0] - int(l.reshape(-1, 2)[-1, 0]), q[1] - int(l.reshape(-1, 2)[-1, 1])) == v for q, l in zip(taps[0::2], lines[0::2]))


def test_chain_moves_the_cursor():
    lines, taps, R = SMALL["chain"]
    ev = [e for e in model("chain")[1] if e["ev"] == "drain"]
    assert [e["t"] for e in ev] == [0, 1, 2, 3, 4] and len({e["run"] for e in ev}) == 1
    assert ev[0]["from"] == C.CHAIN_E and all(math.hypot(t[0] - C.CHAIN_E[0], t[1] - C.CHAIN_E[1]) > R for t in taps[1:])
    assert all(e["from"] == taps[e["t"] - 1] for e in ev[1:])


def test_pass_is_forward_only():
    lines, taps, R = SMALL["forward_only"]
    assert [tuple(int(v) for v in r) for r in rows("forward_only")] == [(0, 0, 0, 0, 0), (1, -1, 0) + taps[1], (0, 1, 0, 0, 0), (1, -1, 0) + taps[0]]
    tr = model("forward_only")[1]
    assert [e["t"] for e in tr if e["ev"] == "drain"] == [1]
    assert math.hypot(taps[0][0] - taps[1][0], taps[0][1] - taps[1][1]) <= R          # within R of the cursor once tap 1 is drained
    assert [e for e in tr if e["ev"] == "pick" and e["idx"] == 2 * len(lines) + 0]    # and yet it comes through the nearest search, after line 1


def test_chunk_boundaries():
    lines, taps, R, hits = C.chunk_case()
    ev = [e for e in model("chunks")[1] if e["ev"] == "drain"]
    assert [e["t"] for e in ev] == hits and [e["offset"] for e in ev] == C.CHUNK_OFFSETS and len({e["run"] for e in ev}) == 1
    assert {0, 63, 64, 1023, 1024} <= set(C.CHUNK_OFFSETS) and max(C.CHUNK_OFFSETS) > 1024
    assert [(h + 1) % 64 for h in hits[:4]] == [1, 1, 2, 2]          # the pass goes on from starts that are no multiple of 64
    far = [t for i, t in enumerate(taps) if i not in hits]
    assert len(far) == sum(C.CHUNK_OFFSETS) + 10 and all(math.hypot(t[0] - 800, t[1] - 10) > 20000 for t in far)      # alive and out of reach all along


# ---------------------------------------------------------------- A.3, A.4, A.5
TIES = {"tie_start_end": [(1, [2, 3]), (2, [4, 5])], "tie_end_j_start_k": [(1, [3, 4])], "tie_line_tap": [(1, [2, 4])], "tie_two_taps": [(1, [2, 3])],
        "tie_5_0_3_4": [(1, [1, 2])], "tie_3_4_5_0": [(1, [1, 2])], "tie_25_15_7": [(1, [1, 2, 3])], "tie_7_15_25": [(1, [1, 2, 3])],
        "duplicates": [(1, [2, 4]), (3, [6, 7])], "first_taps_tie": [(0, [0, 1, 2])]}


@pytest.mark.parametrize("name", sorted(TIES))
def test_ties_are_ties(name):
    """at op number nops the candidates listed (2 k / 2 k + 1: start / end of line k; 2 nl + t: tap t) are at the same, least d^2 and the first of them is taken"""
    picks = {e["nops"]: e for e in model(name)[1] if e["ev"] == "pick"}
    for nops, ties in TIES[name]:
        assert picks[nops]["ties"] == ties and picks[nops]["idx"] == ties[0], (nops, picks[nops])


def test_first_op_claims():
    f = model("first_equal_len")[1][0]
    assert f["ev"] == "first" and f["k"] == 0 and f["same_len"] == [0, 1, 2]
    lines, taps, _ = SMALL["first_long_poly"]
    assert lines[1].shape[0] == C.LONG_POINTS > 192 and model("first_long_poly")[1][0]["k"] == 1 and tuple(rows("first_long_poly")[0]) == (0, 1, 0, 0, 0)
    assert O.build_ops12(lines, taps)[0]["points"].shape == (C.LONG_POINTS, 2)
    p = SMALL["first_ends_equal"][0][0].reshape(-1, 2)
    assert p[0] @ p[0] == p[-1] @ p[-1] and not np.array_equal(p[0], p[-1])
    p = SMALL["first_end_nearer"][0][0].reshape(-1, 2)
    assert p[-1] @ p[-1] < p[0] @ p[0]
    assert (0, 0) in SMALL["first_tap_on_origin"][1] and SMALL["first_tap_on_origin"][1][0] != (0, 0)


def test_degenerate_and_signed_claims():
    assert len(rows("empty")) == 0 and len(rows("one_point_alone")) == 0
    lines, taps, _ = SMALL["one_point_line"]
    assert [p.shape[0] for p in lines] == [2, 1, 2] and len(rows("one_point_line")) == len(lines) + len(taps) - 1
    assert all(p.shape[0] == 1 for p in SMALL["one_point_lines_only"][0])
    lines, taps, _ = SMALL["signed"]
    xy = np.concatenate([np.concatenate([p.reshape(-1, 2) for p in lines]), np.array(taps)])
    assert (xy.min(0) < -2000).all() and (xy.max(0) > 2000).all()
    assert any(e["ev"] == "drain" for e in model("signed")[1])


# ---------------------------------------------------------------- A.6
@pytest.mark.parametrize("name", sorted(C.LDS_CASES))
def test_lds_limit(name):
    """438 taps put the lists 6 bytes over the wave kernel's LDS limit, 437 leave them 3 bytes under; the oracle's answer has passes that drain"""
    nl, nt = C.LDS_CASES[name]
    assert (C.lds_bytes(nl, nt) > C.LDS_LIMIT) == (name == "lds_over")
    assert abs(C.lds_bytes(nl, nt) - C.LDS_LIMIT) <= 9
    lines, taps, R = C.lds_case(name)
    assert (len(lines), len(taps)) == (nl, nt) and all(p.shape[0] == 2 for p in lines)
    w = O.ops12_raw(lines, taps, R)
    assert len(w) == nl + nt
    assert ((w[1:, 0] == 1) & (w[:-1, 0] == 1)).any()          # taps in a row: only a pass emits those while lines are left


# ---------------------------------------------------------------- A.7
@pytest.mark.parametrize("name", sorted(C.WIDE))
def test_wide_cases(name):
    lines, taps, R = SMALL[name]
    xy = np.concatenate([p.reshape(-1, 2) for p in lines] + [np.array(taps, np.int64).reshape(-1, 2)]).astype(np.int64)
    assert np.abs(xy).max() <= C.COORD_MAX
    span = int(max(xy.max(0).max(), 0) - min(xy.min(0).min(), 0))
    assert 2 * span * span >= 1 << 32                                   # past the packed key
    wrapped = C.model(lines, taps, R, wrap=True)[0]
    assert not np.array_equal(wrapped, rows(name))                      # and the packed key's wrap changes the answer
    if name.startswith("wide_2p") or name.startswith("wide_pm"):
        assert span == {"wide_2p17": 1 << 17, "wide_2p20": 1 << 20, "wide_2p24": 1 << 24, "wide_pm_2p24": 1 << 25}[name]
        assert (xy.max() == {"wide_2p17": 1 << 17, "wide_2p20": 1 << 20}.get(name, 1 << 24)) and (xy.min() == (-(1 << 24) if name == "wide_pm_2p24" else 0))
        # the choice at the far corner: the model's pick is 1500 px away, the wrapped key's is a candidate whose d^2 is a multiple of 2^32
        first = [e for e in C.model(lines, taps, R)[1] if e["ev"] == "pick"][0]
        wfirst = [e for e in C.model(lines, taps, R, wrap=True)[1] if e["ev"] == "pick"][0]
        assert first["d2"] == 1500 ** 2 and wfirst["d2"] % (1 << 32) == 0 and wfirst["d2"] >= 1 << 32
        assert any(e["d2"] >= 1 << 32 for e in model(name)[1] if e["ev"] == "pick")      # the exact order itself has to compare distances past 2^32


def test_wide_two_taps_by_hand():
    assert [tuple(int(v) for v in r) for r in rows("wide_two_taps")] == [(1, -1, 0, 30000, 0), (1, -1, 0, 70000, 0)]
    assert (70000 ** 2) % (1 << 32) < 30000 ** 2 < 70000 ** 2
    assert [tuple(int(v) for v in r) for r in rows("wide_tie")] == [(1, -1, 0, 60000, 80000), (1, -1, 0, 0, 100000), (1, -1, 0, 100000, 0)]
    first = [e for e in model("wide_tie")[1] if e["ev"] == "pick"][0]
    assert first["ties"] == [0, 1, 2] and first["d2"] == 10 ** 10 > 1 << 32


def test_refused_cases_are_one_past_the_contract():
    for name, (lines, taps) in C.REFUSED.items():
        xy = np.concatenate([p.reshape(-1, 2) for p in lines] + [np.array(taps, np.int64).reshape(-1, 2)]).astype(np.int64)
        assert np.abs(xy).max() == C.COORD_MAX + 1 and (np.abs(xy) > C.COORD_MAX).sum() == 1, name
