"""Stage 08-A sample production (k_samples) and the per-sample record its consumers read: the smallest shapes at which the mapping of
samples to lanes, the hand-over between threads and blocks, and the packed pixel of a sample can go wrong.  Every case compares
S.dedup_layer with the oracle's stage08_layer, lines and taps, bit-exact.  The sample counts the cases are built for come from the
oracle's own resampling (O.resample_arclen, called the way virtual_draw08 calls it) and are asserted before the GPU runs.

What a kept polyline can be.  split_small keeps a polyline only when its bounding box is at least min_keep (>= 10 px) wide or high
and it is no tap; one that is kept therefore has two distinct points, a positive length, and at least TWO samples (total <= step:
its own >= 2 points pass through; otherwise ceil(total / step) >= 2).  So a layer never has exactly one sample, and no kept
polyline has none: the smallest block-boundary case below is 2 samples, and the polylines "with zero samples" of the mixed case are
the ones the split drops or turns into taps (they sit between the sampled ones in the input list and contribute nothing)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
from util import cfgobj, same_polys, compare_ops


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def P(a):
    return np.asarray(a, np.int32).reshape(-1, 1, 2)


def oracle_samples(polys, cfgd):
    """per input polyline: (number of samples, passes through unresampled), by the oracle's split and resampling (08:127, 08:53-64)"""
    prm = O.derived08(cfgd)
    step = max(1.0, float(cfgd.get("dedup_sample_step", O.DEFAULTS["dedup_sample_step"])))
    out = []
    for p in polys:
        kept, _ = O.split_small_taps08([p], prm)
        if not kept:
            out.append((0, False)); continue
        a = np.asarray(kept[0]).reshape(-1, 2); n = len(a)
        if n >= 2 and (a[0] == a[n - 1]).all():
            n -= 1
        if n < 2:
            out.append((0, False)); continue
        f = a[:n].astype(np.float32)
        S, ps = O.resample_arclen(f, bool(n > 2 and (f[0] == f[n - 1]).all()), step)
        out.append((len(S) if len(S) >= 2 else 0, ps))
    return out


def check(dev, polys, cfgd):
    from orip import stages as S
    want_l, want_t = O.stage08_layer(polys, O.derived08(cfgd))
    got_l, got_t = S.dedup_layer(polys, cfgobj(cfgd), dev)
    assert got_t == want_t
    assert same_polys(got_l, want_l), (len(got_l), len(want_l))


CFG6 = dict(O.DEFAULTS, pixels_per_mm=6)          # canvas 1260 x 1782
# sampling every 40 px: the stage wants 2 * dedup_sample_step < max_join_jump_px (default 80), and below that bound the jump changes no result
CFG6_STEP40 = dict(CFG6, dedup_sample_step=40, max_join_jump_px=120.0)


# ---------------------------------------------------------------- 1. block-size boundaries
def straight_lines(total, step):
    """horizontal two-point polylines, 40 px apart, of at most 140 samples each and `total` samples together (a line of m samples is step * m - step / 2 long)"""
    out = []; row = 0
    while total > 0:
        m = min(total, 140)
        if 0 < total - m < 4:
            m -= 4                                 # never leave fewer than four samples over: at 8 px a shorter line would be a tap
        L = step * m - step // 2
        out.append(P([[20, 30 + 40 * row], [20 + L, 30 + 40 * row]]))
        total -= m; row += 1
    return out


@pytest.mark.parametrize("count", [2, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_stage08_sample_count_at_block_boundaries(dev, count):
    """sample counts at the edges of a wave's 256 and a block's 1024 samples (2: the smallest layer there is, see the module text; at the default step of 8 px a
    polyline of 2 samples would be a tap, so that case samples every 40 px)"""
    cfgd = CFG6_STEP40 if count == 2 else CFG6
    polys = straight_lines(count, cfgd["dedup_sample_step"])
    ns = oracle_samples(polys, cfgd)
    assert sum(m for m, _ in ns) == count and all(m >= 2 and not ps for m, ps in ns)
    check(dev, polys, cfgd)


# ---------------------------------------------------------------- 2. one polyline over several blocks
def snake(rows=25, width=1150, pitch=40, dx=5):
    pts = []
    for r in range(rows):
        xs = np.arange(40, 40 + width + 1, dx)
        if r & 1:
            xs = xs[::-1]
        pts += [[int(x), 60 + pitch * r] for x in xs]
    return P(pts)


@pytest.mark.parametrize("lead", [False, True])
def test_stage08_one_polyline_spanning_blocks(dev, lead):
    """a snake of ~2 500 samples (step 12): interior blocks whose first sample continues a polyline (the predecessor across the block boundary, both hints
    inside one polyline); with `lead`, a 3-sample polyline goes in front of it in the input"""
    cfgd = dict(CFG6, dedup_sample_step=12)
    polys = ([P([[30, 20], [60, 20]])] if lead else []) + [snake()]
    ns = oracle_samples(polys, cfgd)
    assert 2300 <= ns[-1][0] <= 2700, ns
    if lead:
        assert ns[0] == (3, False)
    check(dev, polys, cfgd)


# ---------------------------------------------------------------- 3. many polylines under one wave
def mixed_short(n=300, seed=5):
    """n sampled polylines of 2 .. 5 samples (step 40) on a 72 x 90 lattice, some passing through unresampled; after every third one a polyline that gets
    no sample (too small to keep, or a tap), sometimes several in a row"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        cx, cy = 40 + 72 * (i % 16), 40 + 90 * (i // 16)
        kind = i % 4
        if kind == 0:                                                       # passes through: 26 .. 40 px in 2 .. 5 points
            k = int(rng.integers(2, 6)); L = int(rng.integers(27, 40))
            xs = np.linspace(0, L, k).astype(np.int32)
            out.append(P(np.stack([cx + xs, np.full(k, cy)], 1)))
        else:                                                               # resampled: 41 .. 199 px of a right / down / left / down path: 2 .. 5 samples
            L = int(rng.integers(41, 200))
            pts = [[cx, cy]]
            for lx, ly in ((60, 0), (0, 45), (-60, 0), (0, 34)):
                f = min(1.0, L / (abs(lx) + abs(ly)))
                pts.append([pts[-1][0] + int(lx * f), pts[-1][1] + int(ly * f)])
                L -= int(abs(lx) * f) + int(abs(ly) * f)
                if L <= 0:
                    break
            out.append(P(pts))
        if i % 3 == 0:
            for _ in range(int(rng.integers(1, 4))):
                if rng.random() < 0.5:
                    out.append(P([[cx, cy + 85], [cx + 4, cy + 86]]))                       # below min_keep: dropped
                else:
                    out.append(P([[cx + 5, cy + 84], [cx + 25, cy + 85], [cx + 12, cy + 87]]))     # a tap
    return out


def test_stage08_mixed_short_polylines(dev):
    """a thread's four samples and a wave's 64 cross polyline boundaries all the time"""
    cfgd = CFG6_STEP40
    polys = mixed_short()
    ns = oracle_samples(polys, cfgd)
    sampled = [m for m, _ in ns if m]
    assert len(sampled) == 300 and set(sampled) == {2, 3, 4, 5}, sorted(set(sampled))
    assert sum(1 for m, ps in ns if m and ps) >= 1 and sum(1 for m, ps in ns if m and not ps) >= 1 and sum(1 for m, _ in ns if m == 0) >= 1
    assert sum(sampled) > 512
    check(dev, polys, cfgd)


# ---------------------------------------------------------------- 4. samples off the canvas
def test_stage08_off_canvas_samples(dev):
    """polylines leaving over each edge and coming back, one wholly outside, two reaching beyond +-40 000 (outside 16 bits), one running along the
    last column and the last row with a sample on the corner pixel"""
    cfgd = CFG6
    W, H = O.canvas_size(cfgd)
    polys = [P([[100, 300], [-150, 340], [120, 380]]), P([[W - 100, 500], [W + 150, 540], [W - 120, 580]]),
             P([[400, 100], [440, -150], [480, 120]]), P([[600, H - 100], [640, H + 150], [680, H - 120]]),
             P([[-500, -400], [-100, -300]]),
             P([[200, 900], [45000, 950]]), P([[300, 1000], [-41000, 1100]]), P([[700, 1200], [760, -42000], [820, 1250]]),
             P([[W - 1 - 160, H - 1], [W - 1, H - 1], [W - 1, H - 1 - 160]])]
    ns = oracle_samples(polys, cfgd)
    assert all(m >= 2 for m, _ in ns)
    corner = polys[-1].reshape(-1, 2).astype(np.float32)
    S, _ = O.resample_arclen(corner, False, 8.0)
    assert any(x == W - 1 and y == H - 1 for x, y in S)
    check(dev, polys, cfgd)


# ---------------------------------------------------------------- 5. a retraced cycle
@pytest.mark.parametrize("hooks", [False, True])
def test_stage08_retraced_cycle(dev, monkeypatch, hooks):
    """a 200-point cycle drawn 30 times: the same capsules again and again (de-duplication, first stamp in pop order); with `hooks` the capsule table
    starts too small and the near test goes through the sorted buckets"""
    for k in ("ORIP_CAPS_TINY", "ORIP_HASH_SORT"):
        if hooks:
            monkeypatch.setenv(k, "1")
        else:
            monkeypatch.delenv(k, raising=False)
    a = np.arange(200) * (2 * np.pi / 200)
    cyc = np.stack([600 + 200 * np.cos(a), 800 + 200 * np.sin(a)], 1).astype(np.int32)
    polys = [P(np.concatenate([cyc] * 30 + [cyc[:1]]))]
    ns = oracle_samples(polys, CFG6)
    assert ns[0][0] > 4000
    check(dev, polys, CFG6)


# ---------------------------------------------------------------- 6. walk-coded source
def test_stage08_walk_coded_source(dev):
    """the resident path (stage 08 reads its points from the walk records) with a polyline of 512 or more samples (synth seed 78: the longest has 556;
    seed 77, which test_full_chain_vs_oracle runs at this size, stops at 483)"""
    from orip import stages as S
    from orip.synth import synth_image, layer_names
    K = 8
    img = synth_image(384, 512, K, seed=78)
    cfgd = dict(O.DEFAULTS, color_names=layer_names(K), pixels_per_mm=10)
    want = O.run_pipeline(img, cfgd)
    longest = max(m for n in cfgd["color_names"] for m, _ in oracle_samples(want["sorted"][n], cfgd))
    assert longest >= 512, longest
    ops = S.run_path(img, cfgobj(cfgd), dev)
    compare_ops(ops, want["ops"], cfgd["color_names"])
