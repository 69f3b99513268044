"""BASELINE.json's configurations against the oracle, artefact by artefact, on the DEFAULT A4 canvas (8400 x 11880):

  C1  512 x 512, 4 layers, full path 02 -> 12            (oracle at test time)
      512 x 512, 8 layers, full path                     (the bench image's top-left crop: what bench.py's cpu_baseline times)
  C2  2048 x 2048, 8 layers, stages 02 + 03              (oracle at test time)
  C3  4096 x 4096, 8 layers, full path                   (tests/test_gpu_fullsize.py: SHA-256 digests the oracle left in tests/golden/c3_digests.json)
  K = 16 (C5's layer count) on a small image, full path
  a 2-D grey image (_ensure_bgr, 02:25-30)

Everything is bit-exact: labels, masks, edges, contour / line lists (order included), taps, ops; the plotted path length
(north_star tolerance 1e-3 relative) follows from that and is asserted as well."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
from util import cfgobj as _cfgobj, compare_resident as _compare_resident, compare_ops as _compare_ops


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("case", [(512, 512, 4, "C1"), (512, 512, 8, "bench crop")], ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_full_path_default_canvas_vs_oracle(dev, case):
    """C1 and the 8-layer crop of the bench image: stages 02 -> 12 on the default canvas, every artefact."""
    from orip import stages as S
    from orip.synth import synth_image, layer_names
    H, W, K, _ = case
    img = synth_image(4096, 4096, K)[:H, :W] if K == 8 else synth_image(H, W, K)
    img = np.ascontiguousarray(img)
    cfgd = dict(O.DEFAULTS, color_names=layer_names(K))
    want = O.run_pipeline(img, cfgd)
    ops = S.run_path(img, _cfgobj(cfgd), dev)
    _compare_resident(dev, cfgd, want)
    _compare_ops(ops, want["ops"], cfgd["color_names"])


def test_c2_2048x2048x8_stages_02_03_vs_oracle(dev):
    from orip import stages as S
    from orip.synth import synth_image, layer_names
    H = W = 2048; K = 8
    img = synth_image(H, W, K)
    cfgd = dict(O.DEFAULTS, color_names=layer_names(K))
    want = O.run_pipeline(img, cfgd, upto=3)
    S.run_path(img, _cfgobj(cfgd), dev, upto=3)
    _compare_resident(dev, cfgd, want, upto=3)


def test_k16_full_path_vs_oracle(dev):
    """16 colour layers (BASELINE config 5's layer count, ORIP_MAX_LAYERS) through the whole path."""
    from orip import stages as S
    from orip.synth import synth_image, layer_names
    H, W, K = 320, 384, 16
    img = synth_image(H, W, K, seed=5, sigma=6.0)
    cfgd = dict(O.DEFAULTS, color_names=layer_names(K))
    want = O.run_pipeline(img, cfgd)
    ops = S.run_path(img, _cfgobj(cfgd), dev)
    _compare_resident(dev, cfgd, want)
    _compare_ops(ops, want["ops"], cfgd["color_names"])


def test_gray_2d_input_is_expanded_to_bgr(dev):
    """_ensure_bgr (02:25-30): a 2-D image is processed as the BGR image with three equal channels."""
    from orip import stages as S
    from orip.synth import synth_image, layer_names
    K = 4
    gray = np.ascontiguousarray(synth_image(200, 240, K, seed=11, sigma=5.0)[:, :, 1])
    cfgd = dict(O.DEFAULTS, color_names=layer_names(K), pixels_per_mm=8)
    want = O.run_pipeline(gray, cfgd)          # the oracle's stage02 expands 2-D input the same way
    want3 = O.run_pipeline(np.repeat(gray[:, :, None], 3, axis=2), cfgd, upto=2)
    assert np.array_equal(want["labels"], want3["labels"])
    ops = S.run_path(gray, _cfgobj(cfgd), dev)
    _compare_resident(dev, cfgd, want)
    _compare_ops(ops, want["ops"], cfgd["color_names"])
