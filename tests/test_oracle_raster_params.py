"""The raster sweeps of tests/test_gpu_raster_params.py deserve the name: on the inputs of tests/raster_param_cases.py the oracle alone shows that the
attempt meant to win wins, that the clamps of max_iter and eps sit where the lists assume, that the float32 inputs pass 2^24 and end away from the
exact mean, that equidistant pixels exist, and that every swept iteration count, kernel size and threshold pair changes the result.  CPU only."""
import numpy as np
import pytest

from oracle import oracle as O
import raster_param_cases as C
from util import expected_stage02


def _lab(img):
    return O.bgr2lab(img).reshape(-1, 3).astype(np.float32)


def test_odd_shapes_are_those_of_the_raster_suite():
    import test_gpu_raster
    assert C.ODD_SHAPES == test_gpu_raster.ODD_SHAPES


# ---------------------------------------------------------------- k-means
@pytest.mark.parametrize("seed,K,attempts", C.ATTEMPT_CASES)
def test_last_attempt_wins(seed, K, attempts):
    s = _lab(C.noise_bgr(seed, C.ATTEMPT_SHAPE))
    cen, comp = O.kmeans(s, K, attempts=attempts)
    if attempts > 1:
        cen1, comp1 = O.kmeans(s, K, attempts=attempts - 1)
        assert comp < comp1 and not np.array_equal(cen, cen1)


@pytest.mark.parametrize("seed,K,attempts", C.ATTEMPT_KEEP_CASES)
def test_earlier_attempt_is_kept(seed, K, attempts):
    s = _lab(C.noise_bgr(seed, C.ATTEMPT_SHAPE))
    cen, comp = O.kmeans(s, K, attempts=attempts)
    cen1, comp1 = O.kmeans(s, K, attempts=attempts - 1)
    assert comp == comp1 and np.array_equal(cen, cen1)


def test_equal_attempts_keep_the_first():
    """two colours, K = 2: every attempt ends equally compact, with the colour of its first draw as centre 0; attempt 0 draws another colour than
    attempt 1 (the next group of the device's schedule) and than attempt 4 (its own group), and the oracle keeps attempt 0 whatever follows"""
    img = C.two_colour_bgr(); s = _lab(img)
    first = [tuple(s[i]) for i in C.rng_first_indices(len(s), 2, 8)]
    assert first[1] != first[0] and first[4] != first[0]
    cen1, comp1 = O.kmeans(s, 2, attempts=1)
    assert tuple(np.rint(cen1[0])) == first[0] and tuple(np.rint(cen1[1])) == first[1] and comp1 < 1e-3
    for a in (2, 4, 5, 8):
        cen, comp = O.kmeans(s, 2, attempts=a)
        assert comp == comp1 and np.array_equal(cen, cen1)
    # an attempt whose first draw meets the other colour: the same sample with that draw's position given to a pixel of the other colour.
    # It ends exactly as compact, with the centres the other way round -- so only the order of the attempts keeps attempt 0's centres
    i0 = C.rng_first_indices(len(s), 2, 1)[0]
    j = next(i for i in range(len(s)) if tuple(s[i]) != first[0])
    t = s.copy(); t[[i0, j]] = t[[j, i0]]
    cen_t, comp_t = O.kmeans(t, 2, attempts=1)
    assert comp_t == comp1 and np.array_equal(cen_t, cen1[::-1])


@pytest.fixture(scope="module")
def sweep_sample():
    im = C.SWEEP_IMAGE
    return _lab(C.noise_bgr(im["seed"], im["shape"])), im["K"]


def _groups_hold(results, groups):
    reps = []
    for g in groups:
        for v in g[1:]:
            assert np.array_equal(results[v][0], results[g[0]][0]) and results[v][1] == results[g[0]][1], (g[0], v)
        reps.append(results[g[0]])
    for i in range(len(reps)):
        for j in range(i):
            assert not np.array_equal(reps[i][0], reps[j][0]), (groups[i], groups[j])


def test_max_iter_and_eps_clamps(sweep_sample):
    s, K = sweep_sample
    a, m, e = C.KM_DEFAULT
    by_iter = {v: O.kmeans(s, K, a, v, e) for v in C.MAX_ITERS}
    by_eps = {v: O.kmeans(s, K, a, m, v) for v in C.EPSES}
    assert sorted(sum(C.MAX_ITER_GROUPS, [])) == sorted(C.MAX_ITERS) and sorted(sum(C.EPS_GROUPS, [])) == sorted(C.EPSES)
    _groups_hold(by_iter, C.MAX_ITER_GROUPS)
    _groups_hold(by_eps, C.EPS_GROUPS)
    default = O.kmeans(s, K, a, m, e)
    assert np.array_equal(by_iter[100][0], default[0])                       # 40 iterations are enough here: 100 and 1000 end where the default ends
    assert np.array_equal(by_eps[1e9][0], by_iter[2][0])                     # a large eps stops after the first update, as max_iter 2 does
    assert all(not np.array_equal(by_eps[v][0], default[0]) for v in C.EPSES)
    assert set(C.MAX_ITERS_RGB) <= set(C.MAX_ITERS) and set(C.EPSES_RGB) <= set(C.EPSES)
    zero = O.kmeans(s, K, 0, m, e); one = O.kmeans(s, K, 1, m, e)
    assert np.array_equal(zero[0], one[0]) and zero[1] == one[1]             # attempts < 1 is one attempt


def test_combinations_are_distinct(sweep_sample):
    s, K = sweep_sample
    combos = C.km_combos()
    assert len(combos) == 6 and C.KM_DEFAULT not in combos
    res = [O.kmeans(s, K, *c)[0].tobytes() for c in combos]
    assert len(set(res)) >= 5


@pytest.mark.parametrize("N", C.CHUNK_NS)
def test_chunk_lengths_last_sample_decides(N):
    """the fit of the first N samples is not the fit of the first N - 1: a device that drops the last sample of the last chunk fails the GPU case"""
    im = C.CHUNK_IMAGE
    s = _lab(C.noise_bgr(im["seed"], im["shape"]))
    assert N <= len(s) and N in C.CHUNK_NS and C.CHUNK_N_RGB in C.CHUNK_NS
    assert [-(-n // 16384) for n in C.CHUNK_NS] == [1, 1, 2, 2, 3, 3, 4]
    cen, comp = O.kmeans(s[:N], im["K"], *C.KM_DEFAULT)
    cen1, comp1 = O.kmeans(s[:N - 1], im["K"], *C.KM_DEFAULT)
    assert comp != comp1 or not np.array_equal(cen, cen1)


def test_uniform_image_three_equal_centres():
    s = _lab(np.full((20, 30, 3), (40, 90, 200), np.uint8))
    cen, comp = O.kmeans(s, 3)
    assert comp == 0.0 and np.array_equal(cen, np.repeat(s[:1], 3, axis=0))


def _exact_paths(sums, counts):
    """what a centre update without the float32 accumulation would leave: the rounded true mean, and float32(sum) * (1 / float32(count))"""
    mean = (sums / counts[:, None]).astype(np.float32)
    path = sums.astype(np.float32) * (np.float32(1) / counts.astype(np.float32))[:, None]
    return mean, path


def test_float32_fallback_input_k1():
    s = _lab(C.bright_bgr(C.F32_SIDE_K1))
    cen, _ = O.kmeans(s, 1)
    sums = s.astype(np.int64).sum(0)[None]; counts = np.array([len(s)])
    assert sums[0, 0] == 20526358 and sums[0, 0] >= 1 << 24
    mean, path = _exact_paths(sums, counts)
    assert cen[0, 0] != mean[0, 0] and cen[0, 0] != path[0, 0]
    assert cen[0, 0] == np.float32(228.0703125)
    # the oracle's centre IS the sum in sample order, float32 all the way
    seq = np.cumsum(s, axis=0, dtype=np.float32)[-1] * (np.float32(1) / np.float32(len(s)))
    assert np.array_equal(cen[0], seq)


def _k2_state(side):
    s = _lab(C.bright_bgr(side))
    a, m, e = C.F32_K2_ARGS
    prev, _ = O.kmeans(s, 2, a, m - 1, e)                  # the centres one update earlier: they assign the labels the last update sums
    cen, _ = O.kmeans(s, 2, a, m, e)
    labels = O.assign(s.astype(np.uint8), prev)
    sums = np.array([s[labels == k].astype(np.int64).sum(0) for k in range(2)]); counts = np.bincount(labels, minlength=2)
    return s, prev, cen, labels, sums, counts


def test_float32_fallback_input_k2():
    side = C.F32_SIDE_K2
    assert side * side < 200_000                            # no subsample involved
    s, prev, cen, labels, sums, counts = _k2_state(side)
    assert not np.array_equal(prev, cen)                    # the fit had not stopped earlier, so `labels` are the labels of the last update
    big = sums >= 1 << 24
    assert big.any()
    mean, path = _exact_paths(sums, counts)
    assert (cen != mean)[big].all() and (cen != path)[big].all()
    seq = np.stack([np.cumsum(s[labels == k], axis=0, dtype=np.float32)[-1] * (np.float32(1) / np.float32(counts[k])) for k in range(2)])
    assert np.array_equal(cen, seq)
    assert not (_k2_state(side - 10)[4] >= 1 << 24).any()   # ten pixels less a side and no sum reaches 2^24


# ---------------------------------------------------------------- stage 02
@pytest.mark.parametrize("shape", [s for s in C.SHAPES02 if s[0] * s[1] >= 60], ids=str)
def test_stage02_iteration_pairs_matter(shape):
    img = C.speckle_bgr(shape)
    cen = C.centres_from(O.bgr2lab(img), 3)
    base = expected_stage02(img, cen, 1, 1)
    assert (base[2] > 0).all()                              # every layer holds pixels
    for o, c in C.ITER_PAIRS02:
        assert not np.array_equal(expected_stage02(img, cen, o, c)[3], base[3]), (o, c)


def test_stage02_word_shapes():
    assert [s for s in C.SHAPES02 if s[1] % 64 == 0] == [(5, 64), (64, 64), (8, 128), (33, 192), (5, 256)]
    assert any(s[0] * s[1] < 4 for s in C.SHAPES02) and any(s[0] * s[1] % 4 for s in C.SHAPES02 if s[0] * s[1] > 4)


def test_stage02_tie_inputs():
    img = C.speckle_bgr(C.TIE_SHAPE); lab = O.bgr2lab(img)
    for name, cen in C.tie_centres(lab).items():
        cs, labels, counts, masks = expected_stage02(img, cen, 1, 1)
        if name == "equal_L":
            assert cen[0, 0] == cen[1, 0] and np.array_equal(cs, cen[[2, 0, 1]]) and (counts > 0).all()
        elif name == "identical":
            assert np.array_equal(cen[0], cen[1]) and counts[2] == 0 and not masks[2].any() and counts[0] > 0 and counts[1] > 0    # (layers: centre 2, 0, 1)
        else:
            f = lab.reshape(-1, 3).astype(np.float32)
            d = ((f[:, None, :] - cen[None]) ** 2).sum(2)
            tied = d[:, 0] == d[:, 1]
            assert tied.sum() >= 20
            first = O.assign(lab, cen).ravel()[tied]
            assert (first == 0).all()                       # the first of two equal minima


def test_all_colours_image():
    bgr, rgb = C.all_colours()
    assert bgr.shape == (4096, 4096, 3) and len(np.unique(bgr.reshape(-1, 3).astype(np.uint32) @ np.array([1, 256, 65536], np.uint32))) == 1 << 24
    assert np.array_equal(rgb, bgr.reshape(-1, 3)[:, ::-1])


# ---------------------------------------------------------------- stage 03
@pytest.fixture(scope="module")
def masks03():
    return {kind: f(C.SHAPE03) for kind, f in C.MASK_KINDS.items()}


def test_mask_kinds(masks03):
    assert set(np.unique(masks03["binary"])) == {0, 255}
    g = np.unique(masks03["grey"])
    assert len(g) > 100 and g[0] == 0 and g[-1] == 255
    for shape in C.SHAPES03:
        assert set(np.unique(C.binary_mask(shape))) <= {0, 255}
        if shape[0] * shape[1] > 4:
            assert len(np.unique(C.grey_mask(shape))) > 2


def test_stage03_one_at_a_time_matters(masks03):
    for kind, m in masks03.items():
        base = O.stage03(m, C.cfg03())
        assert base.any()
        for p in [dict(edge_morph_kernel=k) for k in C.MORPH_KERNELS03] + C.ITERS03:
            assert not np.array_equal(O.stage03(m, C.cfg03(p)), base), (kind, p)
        for a, b in C.GAUSS_SAME03:
            assert np.array_equal(O.stage03(m, C.cfg03(dict(edge_kernel_size=a))), O.stage03(m, C.cfg03(dict(edge_kernel_size=b)))), (kind, a, b)
        by_k = [O.stage03(m, C.cfg03(dict(edge_kernel_size=k))) for k in (3, 5, 7)]
        assert not np.array_equal(by_k[0], by_k[1]) and not np.array_equal(by_k[1], by_k[2]) and not np.array_equal(by_k[0], by_k[2])
        assert {k for a, b in C.GAUSS_SAME03 for k in (a, b)} - {3} == set(C.GAUSS_KERNELS03)


def test_stage03_thresholds_matter_on_grey(masks03):
    m = masks03["grey"]
    base = O.stage03(m, C.cfg03())
    res = {t: O.stage03(m, C.cfg03(dict(edge_low_threshold=t[0], edge_high_threshold=t[1]))) for t in C.THRESHOLDS03}
    for t, e in res.items():
        assert not np.array_equal(e, base), t
    a, b = C.THRESHOLD_TWINS03
    assert np.array_equal(res[a], res[b]) and res[a].any()
    # the sweep the raster suite runs on binary masks compares nothing: on a binary mask these pairs are the default result
    mb = masks03["binary"]; bb = O.stage03(mb, C.cfg03())
    assert all(np.array_equal(O.stage03(mb, C.cfg03(dict(edge_low_threshold=lo, edge_high_threshold=hi))), bb) for lo, hi in [(0, 150), (150, 150), (151, 150)])


def test_stage03_combinations(masks03):
    combos = C.combos03()
    assert len(combos) == 8
    for kind, m in masks03.items():
        res = [O.stage03(m, C.cfg03(p)) for p in combos]
        assert sum(bool(e.any()) for e in res) >= 5, kind
        assert len({e.tobytes() for e in res}) >= 5, kind


@pytest.mark.parametrize("shape", [s for s in C.SHAPES03 if s not in ((1, 1), (2, 2))], ids=str)
def test_stage03_shape_sets_matter(shape):
    """at least 7 of the 14 (mask kind, parameter set) cases give a non-empty edge map that is not the default-parameter one"""
    n = 0
    for kind, f in C.MASK_KINDS.items():
        m = f(shape)
        base = O.stage03(m, C.cfg03(C.SHAPE_BASE03))
        for p in C.SHAPE_SETS03.values():
            e = O.stage03(m, C.cfg03(C.SHAPE_BASE03, p))
            n += bool(e.any()) and not np.array_equal(e, base)
    assert n >= 7, (shape, n)


def test_stage03_shapes_straddle_the_switches():
    assert {(7, 7), (7, 8), (8, 7), (8, 8)} <= set(C.SHAPES03)                     # H, W >= 8: the bit-plane NMS
    assert any(s[1] % 64 == 0 and s[0] < 8 for s in C.SHAPES03) and any(s[1] % 64 == 0 and s[0] >= 8 for s in C.SHAPES03)
    assert any(s[0] <= 3 for s in C.SHAPES03) and any(s[1] <= 3 for s in C.SHAPES03)  # a 7-tap Gaussian bounces more than once there


def test_oracle_accepts_what_the_device_refuses(masks03):
    """even and larger structuring elements: the reference passes them to OpenCV, the oracle restates them, the device refuses them (odd, 1..7)"""
    for k in C.REFUSED_MORPH03:
        assert O.stage03(masks03["binary"], C.cfg03(dict(edge_morph_kernel=k))).shape == C.SHAPE03
    for k in C.REFUSED_GAUSS03:
        with pytest.raises(ValueError):
            O.stage03(masks03["binary"], C.cfg03(dict(edge_kernel_size=k)))
