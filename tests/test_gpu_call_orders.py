"""Call orders of the resident chain against the oracle.

liborip.so keeps device state between calls: stage 04's schedule (orip_contours_prepare) and the traces it launches, the walk records of every
layer and their epochs, stage 08's prefetch, slot buffers that only grow.  The other modules feed fresh inputs and run the canonical order;
this one runs the orders a caller may also choose -- a layer traced twice after one prepare, a prepare while traces are still in flight, a
trace after new inputs without a new prepare, stage 08 after its inputs were replaced, lists read after their walk was replaced, one context
across changing shapes, two contexts at once, and the overflow retry of the walk logs -- and holds each result to the oracle, or to a loud
OripError where the order is not allowed.  No leg compares the device with itself.
"""
import re
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
from util import load, same_polys, cfgobj, compare_resident, compare_ops

ODD = [(33, 129), (64, 191)]          # two of test_gpu_raster.ODD_SHAPES: word-boundary widths of the bit planes
PPM = 6                               # a small canvas keeps the oracle's stage 08 quick


@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


def _golden_edges(tag):
    import json
    G = load(f"golden_e2e_{tag}.npz")
    cfg = json.loads(bytes(G["cfg_json"]).decode()); H, W = G["img"].shape[:2]
    return np.stack([np.unpackbits(G[f"edges_{n}"])[:H * W].reshape(H, W) * 255 for n in cfg["color_names"]]).astype(np.uint8)


def _odd_edges(shape):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    return np.stack([(rng.random((H, W)) < d).astype(np.uint8) * 255 for d in (0.08, 0.35, 0.7, 1.0)])


MAPS = {"e2e_a": lambda: _golden_edges("a"), **{f"odd{h}x{w}": (lambda s=(h, w): _odd_edges(s)) for h, w in ODD}}
_want04 = {}


def _edges_and_want(name):
    edges = MAPS[name]()
    if name not in _want04:
        _want04[name] = [O.stage04(e) for e in edges]
    return edges, _want04[name]


def _front_setup(edges):
    from orip import stages as S
    from orip.config import scale_factors
    cfgd = dict(O.DEFAULTS, pixels_per_mm=PPM)
    cfg = cfgobj(cfgd)
    H, W = edges.shape[1:]
    return cfgd, scale_factors(cfg, W, H), S.params08(cfg)


def _want_front(contours, W, H, cfgd):
    """oracle's stages 05 -> 07 -> 08 of one layer"""
    sc = O.stage05(contours, W, H, cfgd)
    so = O.sort07(sc)
    return sc, so, O.stage08_layer(so, O.derived08(cfgd))


def _check_front(dev, l, want_c, want, upto, tag):
    from orip import lib as L
    assert same_polys(dev.get_polys(L.SLOT_CONTOURS, l), want_c), ("contours", tag)
    sc, so, (li, ta) = want
    assert same_polys(dev.get_polys(L.SLOT_SCALED, l), sc), ("scaled", tag)
    if upto >= 8:
        assert same_polys(dev.get_polys(L.SLOT_SORTED, l), so), ("sorted", tag)
        assert same_polys(dev.get_polys(L.SLOT_LINES_INTRA, l), li), ("lines_intra", tag)
        assert dev.get_taps(L.TAPS_INTRA, l) == ta, ("taps_intra", tag)


def _finish_others(dev, K, l):
    """finish the traces prepare launched for the other layers (the next leg starts from a context with nothing in flight)"""
    for k in range(K):
        if k != l:
            dev.contours_layer(k)


def _busiest_layer(want):
    return int(np.argmax([sum(len(p) for p in w) for w in want]))


# ---------------------------------------------------------------- S1: a layer traced again after one prepare
@pytest.mark.parametrize("name", list(MAPS))
def test_retrace_after_one_prepare(dev, name):
    """orip_contours_layer(l) twice, then orip_layer_front(l, ..., 5) twice, then upto=8 after upto=5, all on ONE prepare: every trace of the
    layer must start from unvisited state bytes and a clear memo (trace_launch), so each call gives the oracle's contours again."""
    from orip import lib as L
    edges, want = _edges_and_want(name)
    K, H, W = edges.shape
    cfgd, (sx, sy, dx, dy), p8 = _front_setup(edges)
    dev.set_edges(edges)
    dev.contours_prepare()
    for l in range(K):
        for rep in range(2):
            dev.contours_layer(l)
            assert same_polys(dev.get_polys(L.SLOT_CONTOURS, l), want[l]), (name, l, rep)
    for l in range(K):
        wf = _want_front(want[l], W, H, cfgd)
        for rep in range(2):
            dev.layer_front(l, sx, sy, dx, dy, 5, None)
            _check_front(dev, l, want[l], wf, 5, (name, l, "front5", rep))
        dev.layer_front(l, sx, sy, dx, dy, 8, p8)
        _check_front(dev, l, want[l], wf, 8, (name, l, "front8"))


# ---------------------------------------------------------------- S2: prepare again while a trace is in flight
def _heavy_map(H, W, seed):
    """layer 0: dense noise whose skeleton is one large mesh (a walk of many milliseconds); layers 1-3: a few short strokes"""
    rng = np.random.default_rng(seed)
    e = np.zeros((4, H, W), np.uint8)
    e[0] = (rng.random((H, W)) < 0.4).astype(np.uint8) * 255
    for l in range(1, 4):
        for _ in range(3):
            y, x = int(rng.integers(4, H - 4)), int(rng.integers(4, W - 40))
            e[l, y, x:x + 30] = 255
            e[l, y:y + 20, x] = 255
    return e


@pytest.mark.parametrize("grow", [False, True], ids=["same_size", "growing"])
def test_prepare_again_while_traces_are_in_flight(dev, grow):
    """contours_prepare -> contours_layer(light layers only) -> contours_prepare on the same map (nothing is reallocated) -> every layer.  The
    heavy layer's trace of the first prepare is never finished; the second prepare rewrites the state bytes, keys and chain lists it reads, so it
    must wait for that trace first.  growing: the unfinished trace belongs to a smaller map, and set_edges replaces the edges under it (the
    buffers grow) before the same order runs on the larger map."""
    from orip import lib as L
    if grow:
        dev.set_edges(_heavy_map(480, 512, 3))
        dev.contours_prepare()
        for l in range(1, 4):
            dev.contours_layer(l)
    H, W, seed = (720, 768, 2) if grow else (640, 640, 1)
    edges = _heavy_map(H, W, seed)
    t0 = time.perf_counter()
    want = [O.stage04(e) for e in edges]
    print(f"[call orders] heavy map {H}x{W}: oracle stage 04 {time.perf_counter() - t0:.2f} s, {sum(len(p) for p in want[0])} contour points in the heavy layer")
    dev.set_edges(edges)
    dev.contours_prepare()
    for l in range(1, 4):
        dev.contours_layer(l)
    dev.contours_prepare()
    t0 = time.perf_counter()
    for l in range(4):
        dev.contours_layer(l)
        if l == 0:
            print(f"[call orders] heavy layer: trace + finish {1e3 * (time.perf_counter() - t0):.1f} ms")
    for l in range(4):
        assert same_polys(dev.get_polys(L.SLOT_CONTOURS, l), want[l]), (H, W, l)


# ---------------------------------------------------------------- S3: a trace after new inputs without a new prepare
def _assert_not_stale(dev, l, want_new, tag):
    from orip import lib as L
    from orip.device import OripError
    try:
        dev.contours_layer(l)
    except OripError as e:
        assert "orip_contours_prepare has not run" in str(e), (tag, str(e))
        return
    assert want_new is not None, (tag, "a trace after the inputs were replaced ran on the old schedule")
    assert same_polys(dev.get_polys(L.SLOT_CONTOURS, l), want_new[l]), (tag, l)


def test_trace_after_set_edges_without_prepare(dev):
    """prepare, every layer, then set_edges (new maps, same K and shape) and contours_layer without a new prepare: an OripError or the
    oracle's contours of the NEW edges, never the old ones."""
    a, want_a = _edges_and_want("odd64x191")
    b = np.ascontiguousarray(a[::-1])            # the same densities in the other order: other maps, same K and shape
    want_b = want_a[::-1]
    dev.set_edges(a)
    dev.contours_prepare()
    for l in range(4):
        dev.contours_layer(l)
    dev.set_edges(b)
    for l in range(4):
        _assert_not_stale(dev, l, want_b, ("set_edges", l))


@pytest.mark.parametrize("entry", ["detect_edges", "set_image", "keep_layers", "set_masks", "set_layer_count"])
def test_trace_after_new_raster_inputs_without_prepare(dev, entry):
    """The same after every other entry point that replaces the image, masks, edges or layer count (stages 02 / 03 also use the state bytes'
    buffer as scratch): contours_layer must fail loudly until the next prepare."""
    from orip.synth import synth_image
    H, W, K = 96, 130, 4
    img = synth_image(H, W, K, seed=4, sigma=4.0)
    dev.set_image(img)
    centers, _ = dev.kmeans_fit(None, K)
    dev.extract_layers(centers, want_counts=False)
    masks = np.stack([dev.get_mask(l) for l in range(K)])
    dev.detect_edges()
    dev.contours_prepare()
    for l in range(K):
        dev.contours_layer(l)
    if entry == "detect_edges":
        dev.detect_edges()
    elif entry == "set_image":
        dev.set_image(img)
    elif entry == "keep_layers":
        dev.keep_layers([0, 1])
    elif entry == "set_masks":
        dev.set_masks(masks)
    else:
        dev.set_layer_count(2)
    _assert_not_stale(dev, 0, None, entry)


# ---------------------------------------------------------------- S4: stage 08 after its inputs were replaced
@pytest.mark.parametrize("follow", ["other_params", "shorter_scaled", "rescaled"])
def test_dedup_after_replaced_inputs(dev, follow):
    """layer_front(l, ..., 8) computes stage 08's order-independent part under stage 07 (the prefetch, keyed to SORTED by a tag).  A later
    dedup_layer(l) on the same SORTED list -- with other parameters, after SCALED was replaced by a shorter list, after SCALED was rescaled --
    gives the oracle's stage 08 of that SORTED list, or raises the epoch error; never lines built from the replaced list."""
    from orip import lib as L
    from orip import stages as S
    from orip.device import OripError
    edges, want = _edges_and_want("e2e_a")
    K, H, W = edges.shape
    cfgd, (sx, sy, dx, dy), p8 = _front_setup(edges)
    l = _busiest_layer(want)
    sc, so, _ = _want_front(want[l], W, H, cfgd)
    dev.set_edges(edges)
    dev.contours_prepare()
    dev.layer_front(l, sx, sy, dx, dy, 8, p8)
    want_cfg = cfgd
    if follow == "other_params":
        want_cfg = dict(cfgd, pixels_per_mm=PPM + 2)
        prm = S.params08(cfgobj(want_cfg))
    else:
        prm = p8
        if follow == "shorter_scaled":
            short = sc[1:len(sc) // 2 + 1]          # shifted by one polyline: other offsets at every index
            assert len(short) >= 2
            dev.set_polys(L.SLOT_SCALED, l, short)
        else:
            dev.scale_vectors(l, sx * 0.5, sy * 0.5, dx + 3, dy + 1)
    li, ta = O.stage08_layer(so, O.derived08(want_cfg))
    try:
        dev.dedup_layer(l, prm)
    except OripError as e:
        assert follow == "rescaled" and "replaced" in str(e), (follow, str(e))
    else:
        assert same_polys(dev.get_polys(L.SLOT_LINES_INTRA, l), li), follow
        assert dev.get_taps(L.TAPS_INTRA, l) == ta, follow
    _finish_others(dev, K, l)


# ---------------------------------------------------------------- S5: lists built on a replaced walk fail loudly
def test_lists_of_a_replaced_walk_fail_loudly(dev):
    """SCALED and SORTED of layer l stay walk-coded after layer_front(l, ..., 8).  After a new prepare and a new trace of l, reading them,
    sorting SCALED or deduplicating SORTED raises the OripError that names the replaced walk records; a fresh scale of the new contours is the
    oracle's."""
    from orip import lib as L
    from orip.device import OripError
    edges, want = _edges_and_want("e2e_a")
    K, H, W = edges.shape
    cfgd, (sx, sy, dx, dy), p8 = _front_setup(edges)
    l = _busiest_layer(want)
    dev.set_edges(edges)
    dev.contours_prepare()
    dev.layer_front(l, sx, sy, dx, dy, 8, p8)
    dev.contours_prepare()
    dev.contours_layer(l)
    stale = re.compile(r"walk records of layer \d+ .*replaced")
    for what, call in [("get SCALED", lambda: dev.get_polys(L.SLOT_SCALED, l)), ("get SORTED", lambda: dev.get_polys(L.SLOT_SORTED, l)),
                       ("dedup SORTED", lambda: dev.dedup_layer(l, p8)), ("sort SCALED", lambda: dev.sort_contours(l))]:
        with pytest.raises(OripError, match=stale):
            call()
    assert same_polys(dev.get_polys(L.SLOT_CONTOURS, l), want[l])
    dev.scale_vectors(l, sx, sy, dx, dy)
    assert same_polys(dev.get_polys(L.SLOT_SCALED, l), O.stage05(want[l], W, H, cfgd))
    _finish_others(dev, K, l)


# ---------------------------------------------------------------- S6: one context, changing shapes
_want_run = {}


def _image_case(H, W, K, seed=7):
    from orip.synth import synth_image, layer_names
    img = np.ascontiguousarray(synth_image(H, W, K, seed=seed, sigma=5.0))
    cfgd = dict(O.DEFAULTS, color_names=layer_names(K), pixels_per_mm=PPM)
    key = (H, W, K, seed)
    if key not in _want_run:
        _want_run[key] = O.run_pipeline(img, cfgd)
    return img, cfgd, _want_run[key]


def _run_with_hint(d, img, cfgd, hint):
    """run_path's step with contours_reserve given for another image (hint: (image, K)) instead of this one"""
    from orip import stages as S
    cfg = cfgobj(cfgd)
    names = list(cfg.color_names); K = max(2, len(names)); lnames = S.cluster_names(cfg)[:K]
    H, W = img.shape[:2]
    d.set_image(hint[0])
    d.contours_reserve(hint[1])
    d.set_image(img)
    centers, _ = d.kmeans_fit(S.subsample_indices(H * W), K)
    d.extract_layers(np.asarray(centers, np.float32), want_counts=False)
    S._detect_edges_resident(d, cfg)
    order = sorted(range(K), key=lambda l: (S.darkness_rank10(lnames[l]), names.index(lnames[l])))
    R = S.r_insert12(cfg)
    res = S.run_layer_pipelines(d, cfg, W, H, range(K), order, 12, lambda l: S.ops_from_device(d, l, R))
    return {lnames[l]: res[l] for l in range(K)}


def test_one_context_changing_shapes():
    """A fresh context through steps whose sizes shrink and grow (every slot buffer only grows), then steps whose contours_reserve hint names
    another layer count or another image size: every step equals the oracle, artefact by artefact and in ops."""
    from orip import stages as S
    from orip.device import Device
    d = Device(0)
    try:
        for H, W, K in [(512, 512, 8), (64, 1030, 3), (300, 300, 16), (33, 129, 2), (512, 512, 8)]:
            img, cfgd, want = _image_case(H, W, K)
            ops = S.run_path(img, cfgobj(cfgd), d)
            compare_resident(d, cfgd, want)
            compare_ops(ops, want["ops"], cfgd["color_names"])
        big, _, _ = _image_case(512, 512, 8)
        for (H, W, K), hint in [((300, 300, 16), (None, 2)), ((64, 1030, 3), (big, 16)), ((512, 512, 8), (None, 16))]:
            img, cfgd, want = _image_case(H, W, K)
            ops = _run_with_hint(d, img, cfgd, (img if hint[0] is None else hint[0], hint[1]))
            compare_resident(d, cfgd, want)
            compare_ops(ops, want["ops"], cfgd["color_names"])
    finally:
        d.close()


# ---------------------------------------------------------------- S7: two contexts at once (bench.py's pipelined leg)
def test_two_contexts_at_once():
    """Two contexts, one host thread each, three steps each of run_path_sharded(d, cfg, H, W, 0, 1) on different images -- what the bench's
    "two images in flight" leg runs.  Every step's LINES_CROSS, TAPS_CROSS and ops of every layer equal the oracle's, for both contexts."""
    from orip import lib as L, parallel as P, stages as S
    from orip.device import Device
    cases = [(384, 512, 8), (512, 512, 5)]
    prepared = [_image_case(H, W, K, seed=9) for H, W, K in cases]
    devs = [Device(0), Device(0)]
    got = [[], []]
    errors = []

    def work(i):
        d = devs[i]; img, cfgd, _ = prepared[i]; H, W = img.shape[:2]
        cfg = cfgobj(cfgd); R = S.r_insert12(cfg); K = len(cfgd["color_names"])
        try:
            for _ in range(3):
                d.set_image(img)
                P.run_path_sharded(d, cfg, H, W, 0, 1)
                got[i].append([(d.get_polys(L.SLOT_LINES_CROSS, l), d.get_taps(L.TAPS_CROSS, l), S.ops_from_device(d, l, R)) for l in range(K)])
        except BaseException as e:
            errors.append(e)

    try:
        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if errors:
            raise errors[0]
        for i, (img, cfgd, want) in enumerate(prepared):
            lnames = S.cluster_names(cfgobj(cfgd))
            assert len(got[i]) == 3
            for step in got[i]:
                for l, (lines, taps, ops) in enumerate(step):
                    n = lnames[l]
                    assert same_polys(lines, want["cross"][n][0]), (i, n, "lines_cross")
                    assert taps == want["cross"][n][1], (i, n, "taps_cross")
                compare_ops({lnames[l]: step[l][2] for l in range(len(step))}, want["ops"], cfgd["color_names"])
    finally:
        for d in devs:
            d.close()


# ---------------------------------------------------------------- S8: the overflow retry of the walk logs
@pytest.mark.parametrize("f0", [1, 2])
def test_trace_log_overflow_retry(dev, monkeypatch, capfd, f0):
    """ORIP_TRACE_LOG_F=n starts every trace with logs of n entries per skeleton pixel (default 64), so the overflow retry of trace_finish
    (clear the layer's visited bits, trace again with 4x the logs) runs; the contours still equal the oracle's.  ORIP_WALK_DBG reports the
    factor each layer ended with: with n = 1 some must have grown past it."""
    from orip import lib as L
    monkeypatch.setenv("ORIP_TRACE_LOG_F", str(f0))
    monkeypatch.setenv("ORIP_WALK_DBG", "1")
    capfd.readouterr()
    heavy = _heavy_map(256, 256, 5)                 # a dense mesh: its walks log several entries per skeleton pixel
    for name, (edges, want) in [(n, _edges_and_want(n)) for n in MAPS] + [("heavy256", (heavy, [O.stage04(e) for e in heavy]))]:
        dev.set_edges(edges)
        dev.contours_prepare()
        for l in range(edges.shape[0]):
            dev.contours_layer(l)
            assert same_polys(dev.get_polys(L.SLOT_CONTOURS, l), want[l]), (name, l)
    err = capfd.readouterr().err
    factors = [int(f) for f in re.findall(r"\[walk dbg\] layer \d+ NC=\d+ M=\d+ F=(\d+)", err)]
    assert factors and min(factors) >= f0
    if f0 == 1:                                     # (two entries per pixel plus the per-component slack already hold every walk of these maps)
        assert max(factors) > f0, factors
