"""The resident k-means sample set (orip_kmeans_samples / orip_kmeans_samples_info; NULL, -1 of orip_kmeans_fit and orip_kmeans_fit_rgb): a fit from it
equals the fit that uploads the same indices bit for bit, the set survives the stages that rewrite the raster scratch, it is dropped with the first
image of another pixel count and kept for another image of the same one.  The second image is SMALLER on purpose: a set that was not dropped would
read stale pixels of the larger buffer and give other centres; it would not fault."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, LIMIT = 80, 96, 2_000
H2, W2 = 48, 64


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


@pytest.mark.parametrize("rgb", [False, True], ids=["lab", "rgb"])
def test_resident_fit_through_its_lifetime(dev, rgb):
    from orip import stages as S
    from orip.device import RESIDENT, OripError
    fit = dev.kmeans_fit_rgb if rgb else dev.kmeans_fit
    dev.kmeans_samples(None)
    assert dev.kmeans_samples_info() == (0, 0)
    dev.set_image(_img(H, W, 1))
    idx = S.subsample_indices(H * W, LIMIT)
    assert len(idx) == LIMIT
    for K in (2, 5):
        up = fit(idx, K)                                                         # today's path: the indices uploaded by the call
        dev.kmeans_samples(idx)
        assert dev.kmeans_samples_info() == (LIMIT, H * W)
        assert _same(fit(RESIDENT, K), up), K
        # the stages that rewrite tmpA .. tmpD, the state bytes among them: the set does not live in stage scratch
        dev.extract_layers(up[0], want_counts=False)
        dev.detect_edges()
        dev.contours_prepare()
        assert _same(fit(RESIDENT, K), up), K
        assert dev.kmeans_samples_info() == (LIMIT, H * W)
    # ---- a smaller image: the set is gone
    small = _img(H2, W2, 2)
    dev.set_image(small)
    assert dev.kmeans_samples_info() == (0, 0)
    with pytest.raises(OripError) as e:
        fit(RESIDENT, 3)
    assert "0 indices" in str(e.value) and f"{H2 * W2} pixels" in str(e.value), str(e.value)
    idx2 = S.subsample_indices(H2 * W2, LIMIT)
    up2 = fit(idx2, 3)
    assert _same(dev.kmeans_fit_subsampled(LIMIT, 3, *((3, 30, 1.0) if rgb else ()), rgb=rgb), up2)      # builds the set of (H2 W2, LIMIT) ...
    assert dev.kmeans_samples_info() == (LIMIT, H2 * W2)
    assert _same(dev.kmeans_fit_subsampled(LIMIT, 3, *((3, 30, 1.0) if rgb else ()), rgb=rgb), up2)      # ... and finds it there
    # ---- a set made for another pixel count is named in the message
    dev.set_image(_img(H, W, 1))
    assert dev.kmeans_samples_info() == (0, 0)
    dev.kmeans_samples(idx)
    dev.set_edges(np.zeros((1, H2, W2), np.uint8))                                # H, W of the context change, the image does not: no fit from the set
    with pytest.raises(OripError) as e:
        fit(RESIDENT, 3)
    assert f"{LIMIT} indices made for {H * W} pixels" in str(e.value) and f"{H2 * W2} pixels" in str(e.value), str(e.value)
    # ---- another image of the same size keeps the set
    other = _img(H, W, 3)
    dev.set_image(other)
    assert dev.kmeans_samples_info() == (LIMIT, H * W)
    assert _same(fit(RESIDENT, 4), fit(idx, 4))
    # ---- below the limit kmeans_fit_subsampled fits every pixel and uploads nothing
    dev.kmeans_samples(None)
    assert _same(dev.kmeans_fit_subsampled(H * W, 2, *((3, 30, 1.0) if rgb else ()), rgb=rgb), fit(None, 2))
    assert dev.kmeans_samples_info() == (0, 0)


def test_indices_outside_the_image_are_refused(dev):
    from orip.device import OripError
    dev.set_image(_img(H2, W2, 4))
    dev.kmeans_samples(np.arange(10, dtype=np.int64))
    for bad in ([0, H2 * W2], [-1, 3]):
        with pytest.raises(OripError):
            dev.kmeans_samples(np.array(bad, np.int64))
        assert dev.kmeans_samples_info() == (0, 0)
