"""analyze_colors on the GPU (csrc/analyze.hip) on the cases of tests/analyze_cases.py, against the numpy double (tests/analyze_double.py), bit for bit and without
tolerance: tables past one pass of the capped grids and past 256 seeding segments, seeds steered onto the edges of the two-level search and directly in front
of zero weights, Lloyd at ties, around the host's look every 8 iterations, at the argument limits, with heavy weights and with an emptied cluster, the
compaction at its bin edges and on every colour there is, the filter at equality, and the hue bucket of each of the 2^24 colours.
tests/test_analyze_cases_host.py shows that each case reaches what it is named after."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analyze_cases as A
import analyze_double as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "golden_analyze.npz"))


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def _set_rgb(dev, rgb):
    dev.set_image(np.ascontiguousarray(np.asarray(rgb, np.uint8)[:, :, ::-1]))


def _check_table(dev, rgb, **kw):
    """table, kept pixels, flag and the eleven hue counts against the double -> the double's (keys, counts)"""
    _set_rgb(dev, rgb)
    keys, counts, kept, used_all = dev.colors_table(**kw)
    wk, wc, wkept, wall = D.color_table(rgb, **kw)
    assert keys.dtype == np.uint32 and counts.dtype == np.int64
    assert (kept, used_all) == (wkept, wall), kw
    assert np.array_equal(keys, wk) and np.array_equal(counts, wc), kw
    want_hue = D.hue_counts_np(wk, wc)
    if len(wk) <= 4096:
        assert want_hue.tolist() == D.hue_counts(wk, wc).tolist()
    assert dev.colors_hue().tolist() == want_hue.tolist(), kw
    return wk, wc


def _check_kmeans(dev, keys, counts, K, best=True, **kw):
    """every init of colors_kmeans on the resident table against the double"""
    from orip.analyze import best_init
    cen, n, sums, it = dev.colors_kmeans(K, **kw)
    wcen, wn, wsums, wit = D.kmeans(keys, counts, K, **kw)
    assert it.tolist() == wit.tolist()
    assert np.array_equal(n, wn) and np.array_equal(sums, wsums)
    assert cen.dtype == np.float64 and cen.tobytes() == wcen.tobytes()
    if best:
        assert best_init(n, sums) == D.best_init(keys, counts, wn, wsums)
    return cen, n, sums, it


def _small(dev, keys, counts=None):
    """a table given as keys (and counts) -> resident on the device, checked"""
    counts = np.ones(len(keys), np.int64) if counts is None else counts
    wk, wc = _check_table(dev, A.weighted_image(keys, counts), ignore_white=False)
    assert wk.tolist() == sorted(keys) and wc.tolist() == [c for _, c in sorted(zip(keys, np.asarray(counts).tolist()))]
    return wk, wc


# ---- 1. tables past one pass of the grid and past 256 segments
@pytest.mark.parametrize("name", list(A.BIG))
def test_big_table_hue_and_kmeans(dev, name):
    keys, counts = _check_table(dev, A.distinct_image(name), ignore_white=False)
    assert len(keys) == A.BIG[name][1]
    _check_kmeans(dev, keys, counts, **A.BIG_KMEANS)


# ---- 2. steered seeding
@pytest.fixture(scope="module")
def steer_table():
    keys, counts, _, _ = D.color_table(A.distinct_image(A.STEER_TABLE), ignore_white=False)
    return keys, counts


@pytest.mark.parametrize("want", list(A.STEER))
def test_steered_first_seed(dev, steer_table, want):
    keys, counts = steer_table
    _set_rgb(dev, A.distinct_image(A.STEER_TABLE))
    assert dev.colors_table(ignore_white=False, fetch=False)[2] == A.STEER_D
    seed = A.STEER[want][0]
    assert D.seed_indices(keys, counts, A.STEER_KMEANS["K"], seed, 0)[0] == want
    _check_kmeans(dev, keys, counts, best=False, seed=seed, **A.STEER_KMEANS)


@pytest.mark.parametrize("keys,K,seed,hit", A.ZERO_WEIGHT + A.ZERO_TAIL)
def test_seeding_steps_over_zero_weights(dev, keys, K, seed, hit):
    wk, wc = _small(dev, keys)
    for max_iter in (1, 300):                                                                     # one iteration: n and the sums show the seeds themselves
        _check_kmeans(dev, wk, wc, K, n_init=1, max_iter=max_iter, seed=seed)


# ---- 3. Lloyd at its edges
@pytest.mark.parametrize("name", list(A.TIES))
def test_ties_go_to_the_lower_index(dev, name):
    keys, mid, seeds = A.TIES[name]
    wk, wc = _small(dev, keys)
    for seed, chosen in seeds.items():
        cen, n, sums, it = _check_kmeans(dev, wk, wc, 2, n_init=1, max_iter=1, seed=seed)
        k = np.array(keys, np.int64)[[mid, chosen[0]]]
        assert n[0].tolist() == [2, 1] and sums[0, 0].tolist() == [int((k >> 16).sum()), int(((k >> 8) & 255).sum()), int((k & 255).sum())]
        _check_kmeans(dev, wk, wc, 2, n_init=3, max_iter=300, seed=seed)


@pytest.fixture(scope="module")
def look_tables():
    return {img: D.color_table(G[f"img_{img}"])[:2] for img in {v[0] for v in A.LOOK_CASES.values()}}


@pytest.mark.parametrize("max_iter", A.LOOK_MAX_ITER)
@pytest.mark.parametrize("name", list(A.LOOK_CASES))
def test_one_init_frozen_while_the_other_runs_on(dev, look_tables, name, max_iter):
    img, K, seed, full = A.LOOK_CASES[name]
    keys, counts = look_tables[img]
    _set_rgb(dev, G[f"img_{img}"])
    assert dev.colors_table(fetch=False)[2] == int(counts.sum())
    cen, n, sums, it = _check_kmeans(dev, keys, counts, K, n_init=2, max_iter=max_iter, seed=seed)
    assert it.tolist() == [min(f, max_iter) for f in full]


def test_both_compile_time_maxima_at_once(dev):
    keys, counts = _check_table(dev, A.limits_image())
    cen, n, sums, it = _check_kmeans(dev, keys, counts, A.MAXK, n_init=A.MAX_INIT, max_iter=20)
    assert cen.shape == (A.MAX_INIT, A.MAXK, 3)


def test_argument_errors(dev):
    from orip.device import OripError
    _check_table(dev, A.limits_image())
    with pytest.raises(ValueError, match="n_init=0"):
        dev.colors_kmeans(2, n_init=0)
    with pytest.raises(OripError, match="n_init=65 out of range 1..64"):
        dev.colors_kmeans(2, n_init=65)
    with pytest.raises(OripError, match="max_iter=0 must be at least 1"):
        dev.colors_kmeans(2, max_iter=0)
    keys, counts, _, _ = D.color_table(A.limits_image())
    _check_kmeans(dev, keys, counts, 2, n_init=2)                                                 # the refused calls left the table and the context as they were


def test_heavy_weights(dev):
    keys, counts = _check_table(dev, A.heavy_image(), ignore_white=False)
    assert len(keys) == 5
    for seed in (42, 0, 3):
        cen, n, sums, it = _check_kmeans(dev, keys, counts, 2, n_init=4, max_iter=50, seed=seed)
    assert sums.max() > 10 ** 8


@pytest.mark.parametrize("max_iter", A.EMPTY_MAX_ITER)
@pytest.mark.parametrize("name", list(A.EMPTY_CLUSTER))
def test_an_emptied_cluster_keeps_its_centre(dev, name, max_iter):
    keys, counts, K, seed, at, k, n_final = A.EMPTY_CLUSTER[name]
    wk, wc = _small(dev, keys, np.array(counts, np.int64))
    cen, n, sums, it = _check_kmeans(dev, wk, wc, K, n_init=1, max_iter=max_iter, seed=seed)
    assert (n[0, k] == 0) == (max_iter == at or (max_iter > at and n_final[k] == 0))


# ---- 4. the table kernels
def test_compaction_at_its_bin_edges(dev):
    img = A.edge_image()
    keys, counts = _check_table(dev, img, ignore_white=False)
    assert keys.tolist() == A.EDGE_KEYS and counts.tolist() == A.EDGE_COUNTS
    keys, counts = _check_table(dev, img)
    white = A.is_white(A.EDGE_KEYS)
    assert keys.tolist() == [k for k, w in zip(A.EDGE_KEYS, white) if not w] and counts.tolist() == [c for c, w in zip(A.EDGE_COUNTS, white) if not w]


def test_every_colour_there_is(dev):
    """the expected values are arithmetic: keys = 0 .. 2^24 - 1, counts 1; the default filter drops the 16^3 colours with every channel >= 240"""
    buckets = A.every_colour_buckets()
    _set_rgb(dev, A.every_colour_image())
    keys, counts, kept, used_all = dev.colors_table(ignore_white=False)
    assert len(keys) == kept == A.AN_BINS and not used_all
    assert np.array_equal(keys, np.arange(1 << 24, dtype=np.uint32)) and (counts == 1).all()
    assert dev.colors_hue().tolist() == np.bincount(buckets, minlength=11).tolist()
    keys, counts, kept, used_all = dev.colors_table()
    nonwhite = ~A.is_white(np.arange(1 << 24))
    assert len(keys) == kept == (1 << 24) - 16 ** 3 == 16773120 and not used_all
    assert np.array_equal(keys, np.flatnonzero(nonwhite).astype(np.uint32)) and (counts == 1).all()
    assert dev.colors_hue().tolist() == np.bincount(buckets[nonwhite], minlength=11).tolist()


def test_filter_decides_at_equality(dev):
    keys, counts = _check_table(dev, A.filter_image(100))
    assert int(counts.sum()) == 100 and not A.is_white(keys).any()
    keys, counts = _check_table(dev, A.filter_image(99))
    assert int(counts.sum()) == 256 and A.is_white(keys).any()
    _set_rgb(dev, A.filter_image(99))
    assert dev.colors_table()[2:] == (256, True) and dev.colors_table(min_kept=99)[2:] == (99, False) and dev.colors_table(min_kept=100)[2:] == (256, True)


@pytest.mark.parametrize("thr", list(A.THRESHOLDS))
def test_thresholds(dev, thr):
    img = A.threshold_image()
    keys, counts = _check_table(dev, img, white_threshold=thr, min_kept=1)
    want = sorted(r << 16 | g << 8 | b for r, g, b in A.THRESHOLDS[thr])
    assert keys.tolist() == (want or sorted(r << 16 | g << 8 | b for r, g, b in A.THRESHOLD_COLOURS))
    _check_table(dev, img, ignore_white=False, white_threshold=thr, min_kept=10 ** 9)             # the filter switched off: the other two arguments decide nothing


def test_empty_table_and_the_context_afterwards(dev):
    from orip.device import OripError
    for img, kw in ((A.all_white_image(), {"min_kept": 0}), (A.threshold_image(), {"white_threshold": 0, "min_kept": 0})):
        keys, counts = _check_table(dev, img, **kw)
        assert len(keys) == 0 and dev.colors_hue().tolist() == [0] * 11
        with pytest.raises(OripError, match="0 distinct colours are fewer than K=2"):
            dev.colors_kmeans(2)
    keys, counts = _check_table(dev, A.limits_image())                                            # the context still works
    _check_kmeans(dev, keys, counts, 3, n_init=2)


@pytest.mark.parametrize("image", [A.one_colour_tail, A.two_colour_rows, A.three_colour_rows], ids=lambda f: f.__name__)
def test_wave_merging_with_a_partial_last_group(dev, image):
    rgb = image()
    assert rgb.shape[0] * rgb.shape[1] % 4 == 3
    for kw in ({}, {"ignore_white": False}):
        keys, counts = _check_table(dev, rgb, **kw)
        assert int(counts.sum()) == rgb.shape[0] * rgb.shape[1]


# ---- 5. hue, colour by colour
def test_hue_of_the_cube_in_256_slices(dev):
    """slice R holds every (G, B) once: a wrong bucket for a single colour shows unless another colour of the same slice cancels it"""
    buckets = A.every_colour_buckets()
    gb = np.arange(1 << 16, dtype=np.uint32)
    bad = []
    for r in range(256):
        _set_rgb(dev, A.key_image(r << 16 | gb, (256, 256)))
        assert dev.colors_table(ignore_white=False, fetch=False)[2:] == (1 << 16, False)
        if dev.colors_hue().tolist() != np.bincount(buckets[r << 16:(r + 1) << 16], minlength=11).tolist():
            bad.append(r)
    assert bad == []
