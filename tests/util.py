"""Shared helpers for the test-suite (fixtures are flattened polyline lists: *_off, *_pts)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def unflat(g, name):
    off, pts = g[name + "_off"], g[name + "_pts"]
    return [pts[off[i]:off[i + 1]].reshape(-1, 1, 2) for i in range(len(off) - 1)]


def same_polys(a, b):
    if len(a) != len(b):
        return False
    return all(np.array_equal(np.asarray(x).reshape(-1, 2), np.asarray(y).reshape(-1, 2)) for x, y in zip(a, b))


def poly_multiset(polys):
    return sorted(tuple(np.asarray(p).reshape(-1).tolist()) for p in polys)


def cfgobj(d):
    from orip.config import Config
    c = Config()
    for k, v in d.items():
        setattr(c, k, v)
    return c


def compare_resident(dev, cfgd, want, upto=12):
    """every artefact left on the device by S.run_path against the oracle's run_pipeline result"""
    from orip import lib as L, stages as S
    cfg = cfgobj(cfgd)
    lnames = S.cluster_names(cfg)
    assert np.array_equal(dev.get_labels(), want["labels"].astype(np.uint8))
    for l, n in enumerate(lnames):
        assert np.array_equal(dev.get_mask(l), want["masks"][n]), ("mask", n)
        if upto >= 3:
            assert np.array_equal(dev.get_edges(l), want["edges"][n]), ("edges", n)
        if upto < 12:
            continue
        assert same_polys(dev.get_polys(L.SLOT_CONTOURS, l), want["contours"][n]), ("contours", n)
        assert same_polys(dev.get_polys(L.SLOT_SCALED, l), want["scaled"][n]), ("scaled", n)
        assert same_polys(dev.get_polys(L.SLOT_SORTED, l), want["sorted"][n]), ("sorted", n)
        assert same_polys(dev.get_polys(L.SLOT_LINES_INTRA, l), want["intra"][n][0]), ("lines_intra", n)
        assert dev.get_taps(L.TAPS_INTRA, l) == want["intra"][n][1], ("taps_intra", n)
        assert same_polys(dev.get_polys(L.SLOT_LINES_CROSS, l), want["cross"][n][0]), ("lines_cross", n)
        assert dev.get_taps(L.TAPS_CROSS, l) == want["cross"][n][1], ("taps_cross", n)


def compare_ops(ops, want_ops, names):
    from oracle import oracle as O
    for n in names:
        assert len(ops[n]) == len(want_ops[n]), n
        for a, b in zip(ops[n], want_ops[n]):
            assert a["type"] == b["type"]
            if a["type"] == "line":
                assert np.array_equal(a["points"], b["points"]), n
            else:
                assert (a["x"], a["y"]) == (b["x"], b["y"]), n
    dg, tg = O.path_length(ops); dw, tw = O.path_length(want_ops)
    assert abs(dg + tg - dw - tw) <= 1e-3 * (dw + tw)      # north_star: plotted path length within 1e-3 relative


def expected_stage02(img, centres, open_iters, close_iters):
    """stage 02 from explicit centres with any iteration counts, composed from the oracle's parts (O.stage02 fixes the iterations at 1 / 1):
    (centres sorted dark -> light, labels int64 [H,W], pixels per layer, masks uint8 [K,H,W])"""
    from oracle import oracle as O
    cen = np.asarray(centres, np.float32)
    order = np.argsort(cen[:, 0], kind="stable")
    lut = np.zeros(len(cen), np.int64); lut[order] = np.arange(len(cen))
    labels = lut[O.assign(O.bgr2lab(img), cen)]
    masks = np.stack([O.morph_open_close((labels == k).astype(np.uint8) * 255, 0, 3, open_iters, close_iters) for k in range(len(cen))])
    return cen[order], labels, np.bincount(labels.ravel(), minlength=len(cen)), masks
