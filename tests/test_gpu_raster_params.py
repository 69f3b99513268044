"""GPU parity of the raster stages away from their default arguments and at small shapes: the k-means fit (orip_kmeans_fit, orip_kmeans_fit_rgb) over
attempt counts, iteration limits and eps, tiny samples and the float32 accumulation of large clusters; stage 02's assignment and label masks
(orip_extract_layers) over iteration counts, shapes and ties, and the Lab conversion over all 2^24 colours; stage 03 (orip_detect_edges) over
structuring elements, iteration counts, Gaussian kernels and thresholds on binary AND grey masks, at shapes around the kernel switches.
Inputs: tests/raster_param_cases.py; tests/test_oracle_raster_params.py shows on the oracle alone that they do what they were chosen for.
Every comparison is bit exact but the compactness of a fit, which the device sums in another order (1e-9 relative, as in tests/test_gpu_raster.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import raster_param_cases as C
from util import expected_stage02, cfgobj


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def _lab(img):
    return O.bgr2lab(img).reshape(-1, 3).astype(np.float32)


def _fit_matches(dev, sample, idx, K, args=C.KM_DEFAULT, rgb=False):
    want, comp_w = O.kmeans(sample if idx is None else sample[idx], K, *args)
    got, comp_g = (dev.kmeans_fit_rgb if rgb else dev.kmeans_fit)(idx, K, *args)
    assert np.array_equal(got, want), (K, args, got, want)
    assert abs(comp_g - comp_w) <= 1e-9 * max(1.0, abs(comp_w)), (K, args, comp_g, comp_w)


# ---------------------------------------------------------------- k-means
@pytest.mark.parametrize("seed,K,attempts", C.ATTEMPT_CASES + C.ATTEMPT_KEEP_CASES)
def test_kmeans_attempts(dev, seed, K, attempts):
    """the winning attempt at every position of the four-group schedule: a group's first, second and third attempt, with later attempts that lose"""
    img = C.noise_bgr(seed, C.ATTEMPT_SHAPE)
    dev.set_image(img)
    _fit_matches(dev, _lab(img), None, K, (attempts, 40, 0.5))


@pytest.mark.parametrize("attempts", [1, 2, 4, 5, 8])
def test_kmeans_equal_attempts_keep_the_first(dev, attempts):
    """equally compact attempts with the centres in either order: the first one stays, within a group and across groups"""
    img = C.two_colour_bgr()
    dev.set_image(img)
    _fit_matches(dev, _lab(img), None, 2, (attempts, 40, 0.5))


@pytest.fixture(scope="module")
def sweep_image():
    im = C.SWEEP_IMAGE
    return C.noise_bgr(im["seed"], im["shape"]), im["K"]


@pytest.mark.parametrize("max_iter", C.MAX_ITERS)
def test_kmeans_max_iter(dev, sweep_image, max_iter):
    img, K = sweep_image
    dev.set_image(img)
    _fit_matches(dev, _lab(img), None, K, (3, max_iter, 0.5))


@pytest.mark.parametrize("eps", C.EPSES)
def test_kmeans_eps(dev, sweep_image, eps):
    img, K = sweep_image
    dev.set_image(img)
    _fit_matches(dev, _lab(img), None, K, (3, 40, eps))


def test_kmeans_attempts_below_one(dev, sweep_image):
    img, K = sweep_image
    dev.set_image(img)
    _fit_matches(dev, _lab(img), None, K, (0, 40, 0.5))
    _fit_matches(dev, _lab(img), None, K, (-3, 40, 0.5))


@pytest.mark.parametrize("args", C.km_combos(), ids=str)
def test_kmeans_combinations(dev, sweep_image, args):
    img, K = sweep_image
    dev.set_image(img)
    _fit_matches(dev, _lab(img), None, K, args)


@pytest.mark.parametrize("args", [(3, m, 0.5) for m in C.MAX_ITERS_RGB] + [(3, 40, e) for e in C.EPSES_RGB] + [(5, 30, 1.0)], ids=str)
def test_kmeans_rgb_arguments(dev, sweep_image, args):
    """the same fit over the R, G, B bytes (process_colors.py)"""
    img, K = sweep_image
    dev.set_image(img)
    _fit_matches(dev, img[:, :, ::-1].reshape(-1, 3).astype(np.float32), None, K, args, rgb=True)


@pytest.mark.parametrize("K,N", C.TINY_CASES)
def test_kmeans_tiny_samples(dev, K, N):
    img = C.noise_bgr(6, C.ATTEMPT_SHAPE)
    dev.set_image(img)
    idx = C.tiny_indices(K, N)
    _fit_matches(dev, _lab(img), idx, K)
    _fit_matches(dev, img[:, :, ::-1].reshape(-1, 3).astype(np.float32), idx, K, rgb=True)


@pytest.fixture(scope="module")
def chunk_image():
    im = C.CHUNK_IMAGE
    img = C.noise_bgr(im["seed"], im["shape"])
    return img, _lab(img), img[:, :, ::-1].reshape(-1, 3).astype(np.float32), im["K"]


@pytest.mark.parametrize("N", C.CHUNK_NS)
def test_kmeans_chunk_lengths(dev, chunk_image, N):
    """sample counts at which a thread's chunk of samples grows by one (tests/test_oracle_raster_params.py: the last sample decides every one of them)"""
    img, lab, rgb, K = chunk_image
    dev.set_image(img)
    idx = np.arange(N, dtype=np.int64)
    _fit_matches(dev, lab, idx, K)
    if N == C.CHUNK_N_RGB:
        _fit_matches(dev, rgb, idx, K, rgb=True)


def test_kmeans_uniform_image(dev):
    """every distance is 0: three equal centres, compactness 0, two clusters filled by the empty-cluster repair"""
    img = np.full((20, 30, 3), (40, 90, 200), np.uint8)
    dev.set_image(img)
    _fit_matches(dev, _lab(img), None, 3)
    got, comp = dev.kmeans_fit(None, 3)
    assert comp == 0.0 and np.array_equal(got, np.repeat(_lab(img)[:1], 3, axis=0))


def test_kmeans_too_few_samples_is_refused(dev):
    from orip.device import OripError
    img = C.noise_bgr(6, C.ATTEMPT_SHAPE)
    dev.set_image(img)
    with pytest.raises(OripError):
        dev.kmeans_fit(np.array([5, 9], np.int64), 3)
    with pytest.raises(OripError):
        dev.kmeans_fit_rgb(np.array([5, 9], np.int64), 3)
    _fit_matches(dev, _lab(img), None, 6)                   # the same Device goes on


def test_kmeans_float32_accumulation_k1(dev):
    """one cluster whose lightness sum passes 2^24: the centre is the float32 sum in sample order, not the mean (K == 1: one attempt, two iterations)"""
    img = C.bright_bgr(C.F32_SIDE_K1)
    dev.set_image(img)
    _fit_matches(dev, _lab(img), None, 1)
    _fit_matches(dev, _lab(img), None, 1, (4, 100, 0.0))    # K == 1 overrides both


def test_kmeans_float32_accumulation_k2(dev):
    """two clusters, one with a channel sum above 2^24, five centre updates by the serial lane (144 400 samples each).
    Measured on an MI355X: 0.18 s for the whole test, the oracle's fit included -- max_iter stays at the 6 the case was given."""
    img = C.bright_bgr(C.F32_SIDE_K2)
    dev.set_image(img)
    _fit_matches(dev, _lab(img), None, 2, C.F32_K2_ARGS)


# ---------------------------------------------------------------- stage 02
def _stage02_matches(dev, img, cen, o, c):
    cs_w, labels_w, counts_w, masks_w = expected_stage02(img, cen, o, c)
    cs, counts = dev.extract_layers(cen, o, c)
    assert np.array_equal(cs, cs_w), (o, c)
    assert np.array_equal(dev.get_labels(), labels_w.astype(np.uint8)), (o, c)
    assert np.array_equal(counts, counts_w), (o, c)
    for k in range(len(cen)):
        assert np.array_equal(dev.get_mask(k), masks_w[k]), (o, c, k)


@pytest.mark.parametrize("shape", C.SHAPES02, ids=str)
def test_stage02_iterations_and_shapes(dev, shape):
    """label masks after (open, close) other than (1, 1), at shapes with fewer than four pixels, with tail pixels, with and without whole 64-pixel words"""
    img = C.speckle_bgr(shape)
    dev.set_image(img)
    lab = O.bgr2lab(img)
    assert np.array_equal(dev.lab_of(), lab)
    for K in C.KS02:
        cen = C.centres_from(lab, K)
        for o, c in C.ITER_PAIRS02 + [(1, 1)]:
            _stage02_matches(dev, img, cen, o, c)


def test_stage02_masks_feed_stage03(dev):
    """stage 03 starts from the bit planes stage 02 leaves: after iteration counts other than (1, 1) they are still the masks"""
    shape = (33, 192)
    img = C.speckle_bgr(shape)
    dev.set_image(img)
    cen = C.centres_from(O.bgr2lab(img), 3)
    for o, c in [(2, 1), (0, 0), (1, 3)]:
        masks_w = expected_stage02(img, cen, o, c)[3]
        dev.extract_layers(cen, o, c)
        dev.detect_edges(3, 1, 1, 3, 20, 60)
        for k in range(3):
            assert np.array_equal(dev.get_edges(k), O.stage03(masks_w[k], C.cfg03(C.SHAPE_BASE03))), (o, c, k)


def test_stage02_ties(dev):
    """two centres of one lightness keep their order, the second of two identical centres gets nothing, a pixel as far from two centres goes to the first"""
    img = C.speckle_bgr(C.TIE_SHAPE)
    dev.set_image(img)
    for name, cen in C.tie_centres(O.bgr2lab(img)).items():
        _stage02_matches(dev, img, cen, 1, 1)


def test_lab_of_all_colours(dev):
    bgr, rgb = C.all_colours()
    want = O.bgr2lab(bgr)
    dev.set_image(bgr)
    assert np.array_equal(dev.lab_of(), want)
    assert np.array_equal(dev.lab_of_rgb(rgb), want.reshape(-1, 3))


# ---------------------------------------------------------------- stage 03
def _edges_match(dev, masks, cfg):
    dev.set_masks(masks)
    dev.detect_edges(max(1, cfg["edge_morph_kernel"]), cfg["edge_morph_open_iters"], cfg["edge_morph_close_iters"], O.ensure_odd(cfg["edge_kernel_size"]),
                     cfg["edge_low_threshold"], cfg["edge_high_threshold"])
    for k in range(len(masks)):
        assert np.array_equal(dev.get_edges(k), O.stage03(masks[k], cfg)), (cfg, k)


@pytest.fixture(scope="module")
def masks03():
    return {kind: f(C.SHAPE03) for kind, f in C.MASK_KINDS.items()}


@pytest.mark.parametrize("kind", list(C.MASK_KINDS))
@pytest.mark.parametrize("prm", [{}] + C.ONE_AT_A_TIME03 + C.combos03(), ids=str)
def test_stage03_parameters(dev, masks03, kind, prm):
    """a binary mask runs the bit-plane morphology (and the bit-plane NMS under a 3 x 3 Gaussian), a grey one the byte kernels; only on the grey one do
    the thresholds decide anything"""
    _edges_match(dev, masks03[kind][None], C.cfg03(prm))


@pytest.mark.parametrize("kind", list(C.MASK_KINDS))
@pytest.mark.parametrize("shape", C.SHAPES03, ids=str)
def test_stage03_shapes(dev, shape, kind):
    """a 7-tap Gaussian on one to three rows, structuring elements larger than the image, both sides of the H, W >= 8 and W % 64 == 0 switches"""
    m = C.MASK_KINDS[kind](shape)[None]
    for p in list(C.SHAPE_SETS03.values()) + [{}]:
        _edges_match(dev, m, C.cfg03(C.SHAPE_BASE03, p))


def test_stage03_sixteen_layers(dev):
    shape = C.LAYERS_SHAPE03
    masks = np.stack([C.binary_mask(shape, seed=900 + k, t=0.04 * (k - 8)) for k in range(16)])
    _edges_match(dev, masks, C.cfg03(C.SHAPE_BASE03, C.SHAPE_SETS03[C.LAYERS_SET03]))
    grey = np.stack([C.grey_mask(shape, seed=950 + k) for k in range(16)])
    _edges_match(dev, grey, C.cfg03(C.SHAPE_BASE03, C.SHAPE_SETS03[C.LAYERS_SET03]))


def test_stage03_float_thresholds_floor(dev, masks03):
    """S.detect_edges floors float thresholds as cv2.Canny's integer arguments do (50.9 / 150.9 are 50 / 150)"""
    from orip import stages as S
    m = masks03["grey"]
    for lo, hi in ((50.9, 150.9), (49.9, 149.9)):
        cfg = C.cfg03(dict(edge_low_threshold=lo, edge_high_threshold=hi))
        got = S.detect_edges({"layer_dark": m}, cfgobj(cfg), dev)["layer_dark"]
        assert np.array_equal(got, O.stage03(m, cfg)), (lo, hi)
        assert np.array_equal(got, O.stage03(m, C.cfg03(dict(edge_low_threshold=int(lo), edge_high_threshold=int(hi))))), (lo, hi)
    # rounding 49.9 / 149.9 up instead would show: on this mask 50 / 150 is another edge map than 49 / 149 (the magnitudes here are even, so 50.9 alone would not tell)
    assert not np.array_equal(got, O.stage03(m, C.cfg03()))


def test_stage03_refused_kernels(dev, masks03):
    """The device takes odd structuring elements of 1 .. 7 and Gaussians of 3, 5, 7.  The reference hands even and larger structuring elements to OpenCV
    and the oracle restates them; lifting the device's limit is not part of this suite -- what is pinned is the refusal, and that the context works on."""
    from orip.device import OripError
    m = masks03["binary"][None]
    dev.set_masks(m)
    for gk in C.REFUSED_GAUSS03:
        with pytest.raises(OripError):
            dev.detect_edges(3, 1, 1, gk, 50, 150)
    for mk in C.REFUSED_MORPH03:
        with pytest.raises(OripError):
            dev.detect_edges(mk, 1, 1, 3, 50, 150)
    dev.detect_edges()
    assert np.array_equal(dev.get_edges(0), O.stage03(m[0], C.cfg03()))
    _edges_match(dev, masks03["grey"][None], C.cfg03())
