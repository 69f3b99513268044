"""Stage 08-A between k_samples and the acceptance test: the block-local tail sums k_samples leaves for k_tail_par, the first-sample flag in the
packed pixel word that k_caps_insert reads, and the counters that kernels of the chain clear for the ones behind them.  Every case compares
S.dedup_layer with the oracle's stage08_layer, lines and taps, bit-exact; the sample counts the cases are built for come from the oracle's own
resampling and are asserted before the GPU runs (oracle_samples, as in test_gpu_stage08_samples.py).

The shapes.  k_samples sums the distances of the 1024 samples of a block, starting again at the first sample of every polyline; k_tail_par keeps
the 256 sums before its 256 samples and its own in LDS.  So a tail window (tail length / step, in samples) can lie inside the LDS window, reach
below it, or span more than one 1024-block, and a polyline can start anywhere in a block.  The snakes below have rows closer together than the
collision radius (14 px against 18), so a sample is dropped exactly when the sample beside it on the row before has left the tail: the result
depends on the pop count of nearly every sample."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
from util import cfgobj, same_polys


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
    return want_l, want_t


def length(p):
    a = np.asarray(p, np.float64).reshape(-1, 2)
    return float(np.hypot(*(a[1:] - a[:-1]).T).sum())


def rows_path(total, x0, y0, width, pitch, dx=5):
    """a path of rows `width` long, `pitch` apart, left to right and back, a point every dx px, cut off after exactly `total` px (all segments are
    axis-parallel with integer ends, so float32 lengths are exact and a step of 1 px gives `total` samples)"""
    pts = [[x0, y0]]; left = total; r = 0
    while left > 0:
        run = min(width, left); sgn = -1 if r & 1 else 1
        xs = list(range(dx, run, dx)) + [run]
        x_start = pts[-1][0]
        pts += [[x_start + sgn * x, pts[-1][1]] for x in xs]
        left -= run
        if left > 0:
            down = min(pitch, left)
            pts.append([pts[-1][0], pts[-1][1] + down]); left -= down
        r += 1
    return P(pts)


CFG6 = dict(O.DEFAULTS, pixels_per_mm=6)          # canvas 1260 x 1782
SEQ = "ORIP_TAIL_SEQ"


def set_seq(monkeypatch, seq):
    if seq:
        monkeypatch.setenv(SEQ, "1")
    else:
        monkeypatch.delenv(SEQ, raising=False)


# ---------------------------------------------------------------- 1. the tail window against the LDS window and the 1024-sample block
@pytest.mark.parametrize("seq", [False, True])
@pytest.mark.parametrize("step, tail", [(2, 30), (1, 300), (1, 1300)])
def test_stage08_tail_window_sizes(dev, monkeypatch, step, tail, seq):
    """one snake of 3 028 samples (rows of 1 000 px, 14 px apart): a tail of 15 samples (inside the LDS window; a sample every 2 px, so that the tail is
    longer than the collision radius), of 300 (below the window), of 1 300 (over more than one block of k_samples); each also with the sequential
    simulation everywhere"""
    set_seq(monkeypatch, seq)
    cfgd = dict(CFG6, dedup_sample_step=step, ignore_tail_points_intra=tail)
    assert 2 * cfgd["dedup_sample_step"] < cfgd["max_join_jump_px"] and tail > cfgd["collision_radius_intra_px"]
    polys = [rows_path(3028 * step, 40, 60, 1000, 14)]
    assert oracle_samples(polys, cfgd) == [(3028, False)]
    check(dev, polys, cfgd)


def test_stage08_tail_beyond_block_sum_bound(dev, monkeypatch):
    """a tail of 36 000 samples on a polyline of 38 000: the search goes back over more block sums than k_tail_par's error bound allows, so the samples
    mark their polyline and the sequential simulation decides"""
    monkeypatch.delenv(SEQ, raising=False)
    cfgd = dict(CFG6, dedup_sample_step=1, ignore_tail_points_intra=36000)
    polys = [rows_path(38000, 40, 60, 1100, 40, dx=20)]
    assert oracle_samples(polys, cfgd) == [(38000, False)]
    check(dev, polys, cfgd)


# ---------------------------------------------------------------- 2. where the long polyline starts in its block
@pytest.mark.parametrize("leads, snake_len, tail", [((2047,), 1528, 300), ((2048,), 1528, 300), ((2049,), 1528, 300), ((1537, 1536), 1528, 300), ((3071,), 3028, 1300)])
def test_stage08_polyline_start_in_block(dev, monkeypatch, leads, snake_len, tail):
    """longer polylines go first (perimeter, descending), so the snake starts at sample 1023 of a block, at 0 and at 1 of the next one (the block before
    wholly inside ONE other polyline), at 1 behind two polylines, and -- with a tail over more than one block -- at 1023 behind three blocks of another"""
    monkeypatch.delenv(SEQ, raising=False)
    cfgd = dict(CFG6, dedup_sample_step=1, ignore_tail_points_intra=tail)
    snake = rows_path(snake_len, 40, 60, 1000 if snake_len > 2000 else 500, 14)
    lead_polys = [rows_path(L, 60, 300 + 400 * i, 1100, 50, dx=10) for i, L in enumerate(leads)]
    polys = [snake] + lead_polys                          # (the snake first in the input: the order comes from the perimeters)
    assert all(length(l) == L for l, L in zip(lead_polys, leads)) and length(snake) == snake_len and min(leads) > snake_len
    assert sorted(leads, reverse=True) == list(leads)     # stable order: the leads as listed, then the snake
    ns = oracle_samples(polys, cfgd)
    assert ns == [(snake_len, False)] + [(L, False) for L in leads]
    check(dev, polys, cfgd)


# ---------------------------------------------------------------- 3. the first-sample flag: many short polylines
def short_rows(rows=70):
    """five polylines per row on a 2100-px canvas, 40 px between rows.  In processing order (perimeter, descending; the input is in that order): the outer
    columns 0 and 4 in turn, row by row (5 samples each), then columns 1 and 3 in turn (3 .. 4 samples), then the middle column (2 samples).  The straight
    line from the last sample of one polyline to the first sample of the next in that order crosses the columns between them on its way -- polylines
    that come later in the order, that the oracle keeps whole, and that a capsule drawn along that line would have stamped before their turn."""
    out = []
    def line(col, row, L):
        x0 = 60 + 400 * col
        return P([[x0, 50 + 40 * row], [x0 + L, 50 + 40 * row]])
    n = 2 * rows
    for k in range(n):
        out.append(line(0 if k % 2 == 0 else 4, k // 2, 200 - (39 * k) // n))      # 200 .. 162 px: 5 samples at 40 px
    for k in range(n):
        out.append(line(1 if k % 2 == 0 else 3, k // 2, 160 - (79 * k) // n))      # 160 .. 82 px: 4 or 3 samples
    for k in range(rows):
        out.append(line(2, k, 80 - (39 * k) // rows))                             # 80 .. 42 px: 2 samples
    return out


def test_stage08_first_sample_flag_short_polylines(dev):
    """350 polylines of 2 .. 5 samples: threads, waves and blocks cross polyline boundaries all the time, and a capsule from the last sample of one polyline
    to the first of the next would cover samples the oracle keeps: the case is laid out to fail if k_caps_insert ignores the flag (the middle columns would lose lines)"""
    cfgd = dict(O.DEFAULTS, pixels_per_mm=10, dedup_sample_step=40, max_join_jump_px=120.0)      # canvas 2100 x 2970
    polys = short_rows()
    per = [length(p) for p in polys]
    assert per == sorted(per, reverse=True)
    ns = oracle_samples(polys, cfgd)
    assert len(ns) == 350 and {m for m, _ in ns} == {2, 3, 4, 5} and not any(ps for _, ps in ns)
    assert sum(m for m, _ in ns) > 1024
    want_l, want_t = check(dev, polys, cfgd)
    assert sum(len(p) for p in want_l) + len(want_t) > 0


# ---------------------------------------------------------------- 4. the first-sample flag next to high coordinates
def test_stage08_first_sample_flag_high_coordinates(dev):
    """every sample at x, y >= 8192 on the default canvas (8400 x 11880): bit 13 of both coordinates sits next to the flag; the path goes out, comes back
    6 px below itself (dropped where the way out has left the tail) and on"""
    cfgd = dict(O.DEFAULTS)
    assert O.canvas_size(cfgd) == (8400, 11880)
    poly = P([[8200, 8300], [8390, 8300], [8390, 8306], [8200, 8306], [8200, 8400], [8350, 8400]])
    ns = oracle_samples([poly], cfgd)
    assert ns[0][0] >= 60 and not ns[0][1]
    S, _ = O.resample_arclen(poly.reshape(-1, 2).astype(np.float32), False, 8.0)
    r = np.rint(S)
    assert (r >= 8192).all() and (r[:, 0] < 8400).all() and (r[0] == [8200, 8300]).all()
    check(dev, [poly], cfgd)


# ---------------------------------------------------------------- 5. the counters from one call to the next
def test_stage08_counters_across_calls(dev, monkeypatch):
    """on ONE Device, one layer after the other: a layer that overflows a tiny capsule table and leaves survivors for the near test; a layer that does neither
    (no sample ever leaves its polyline's tail, a table with room); a layer with polylines beyond the canvas.  A counter that kept its value from the call
    before would show in the second or third"""
    monkeypatch.delenv(SEQ, raising=False)
    cfgd = CFG6
    W, H = O.canvas_size(cfgd)
    first = [rows_path(24000, 40, 60, 1150, 40, dx=10)]                  # 3 000 samples, 3 000 distinct capsules, nearly every sample a survivor
    assert oracle_samples(first, cfgd) == [(3000, False)]
    second = [P([[100 + 150 * i, 200], [100 + 150 * i, 300]]) for i in range(6)]      # 100 px each: shorter than the tail (120 px), nothing is ever popped
    assert [m for m, _ in oracle_samples(second, cfgd)] == [13] * 6
    third = [P([[100, 300], [-150, 340], [120, 380]]), P([[W - 100, 500], [W + 150, 540], [W - 120, 580]]), P([[600, H - 100], [640, H + 150], [680, H - 120]])]
    assert all(m >= 2 for m, _ in oracle_samples(third, cfgd))
    monkeypatch.setenv("ORIP_CAPS_TINY", "1")
    check(dev, first, cfgd)
    monkeypatch.delenv("ORIP_CAPS_TINY")
    check(dev, second, cfgd)
    check(dev, third, cfgd)
    check(dev, second, cfgd)
