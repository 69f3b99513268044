"""The cases of tests/tail_replay_cases.py hold what they are built for.  k_tail_par's unsure rule (csrc/vector08a.hip) is restated in numpy on the
oracle's own samples: the head of sample j is the smallest h whose tail -- the distances of samples h + 1 .. j -- is at most the tail length T; the sample
is unsure when that tail is not at most T - 1e-6 or, for h > 0, the tail from h - 1 is not above T + 1e-6.  The pop counts come from the reference's
loop (08:139-155) on the same distances.  CPU only."""
import time

import numpy as np
import pytest

from oracle import oracle as O
import tail_replay_cases as C

EPS = 1e-6          # ORIP_TAIL_EPS
BY_ID = {c[0]: c for c in C.CASES}
_memo = {}


def samples_of(cfgd, poly):
    """the oracle's samples of one input polyline (split, resampling: 08:127, 08:53-64), as tests/test_gpu_stage08_chain.py takes their count"""
    prm = O.derived08(cfgd)
    step = max(1.0, float(cfgd["dedup_sample_step"]))
    kept, _ = O.split_small_taps08([poly], prm)
    assert len(kept) == 1
    a = np.asarray(kept[0]).reshape(-1, 2); n = len(a)
    if n >= 2 and (a[0] == a[n - 1]).all():
        n -= 1
    f = a[:n].astype(np.float32)
    S, ps = O.resample_arclen(f, bool(n > 2 and (f[0] == f[n - 1]).all()), step)
    assert not ps
    return np.asarray(S, np.float64)


def study(name):
    """per polyline of the case: (sample count, unsure flags, pops per sample by the reference's loop)"""
    if name not in _memo:
        _, over, polys, _ = BY_ID[name]
        cfgd = dict(O.DEFAULTS, **over); T = float(cfgd["ignore_tail_points_intra"])
        out = []
        for p in polys:
            S = samples_of(cfgd, p)
            d = np.concatenate([[0.0], np.hypot(*(S[1:] - S[:-1]).T)])
            cum = np.cumsum(d)                                        # (exact here: every distance is an integer or one of a few sqrt 2)
            h = np.searchsorted(cum, cum - T, side="left")            # smallest h with cum[j] - cum[h] <= T
            j = np.arange(len(S))
            assert ((cum - cum[h] <= T) & ((h == 0) | (cum - cum[np.maximum(h - 1, 0)] > T))).all()
            unsure = ~(cum - cum[h] <= T - EPS) | ((h > 0) & ~(cum - cum[np.maximum(h - 1, 0)] > T + EPS))
            pops = np.zeros(len(S), np.int64); head = 0; acc = 0.0
            for s in range(len(S)):                                   # 08:139-155
                if s > head:
                    acc += d[s]
                while head <= s and acc > T:
                    head += 1; pops[s] += 1
                    acc = acc - d[head] if head <= s else 0.0
            out.append((len(S), unsure, pops, j))
        _memo[name] = out
    return _memo[name]


@pytest.mark.parametrize("name", [c[0] for c in C.CASES])
def test_case_holds_what_it_is_built_for(name):
    _, over, polys, expect = BY_ID[name]
    cfgd = dict(O.DEFAULTS, **over)
    assert float(cfgd["ignore_tail_points_intra"]) > 0 and len(polys) == len(expect)
    W, H = O.canvas_size(cfgd)
    q = np.concatenate([np.asarray(p).reshape(-1, 2) for p in polys])
    assert q.min() >= 0 and q[:, 0].max() < W and q[:, 1].max() < H
    lengths = [float(np.hypot(*(np.diff(np.asarray(p, np.float64).reshape(-1, 2), axis=0)).T).sum()) for p in polys]
    assert lengths == sorted(lengths, reverse=True), "processing order (perimeter, descending) is the input's"
    for (m, unsure, pops, _), e in zip(study(name), expect):
        assert m == e["samples"]
        n_tail = int(round(float(cfgd["ignore_tail_points_intra"]) / float(cfgd["dedup_sample_step"])))
        if e["unsure"] == "none":
            assert not unsure.any()
            continue
        assert unsure.sum() > 0
        last = int(np.nonzero(unsure)[0][-1])
        if e["unsure"] == "all":
            assert unsure[n_tail:].all() and not unsure[:n_tail].any() and last == m - 1, "unsure from the first full tail to the last sample"
        elif e["unsure"] == "early":
            assert last < m // 4 and m - 1 - last >= 2000 and unsure.sum() > 500, (last, m)
        if "pops" in e:
            s = int(np.argmax(pops))
            assert pops[s] >= e["pops"] and s <= last, "a sample with more than 63 pops, inside the replayed part"


def test_the_oracle_takes_each_case_in_a_few_seconds():
    for name, over, polys, _ in C.CASES:
        t = time.perf_counter()
        O.stage08_layer(polys, O.derived08(dict(O.DEFAULTS, **over)))
        assert time.perf_counter() - t < 5.0, name
