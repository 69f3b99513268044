"""Deterministic inputs for stage 08-B (the skeleton merge) on small canvases whose padded raster puts the stamped bands on the word, tile-column and
tile-row boundaries of the bit-plane kernels.  tests/test_oracle_skel_merge_cases.py (CPU) asserts on the oracle alone that 08-B does something on every
case; tests/test_gpu_skel_merge_cases.py (GPU) compares the device with the oracle.  Plain data and numpy: nothing here touches the oracle or the device.

The padded raster is (W + 128) x (H + 128), 64 px of padding on every side: canvas x = 0 and x = 64 are bit 0 of a word and the first column of a
thinning tile (a tile is 2 words wide); canvas y = 0 and y = 64 are the first row of a tile (64 rows high)."""
import numpy as np


def P(a):
    return np.asarray(a, np.int32).reshape(-1, 1, 2)


# Stage 08-A must leave the near-parallel lines alone, so that 08-B has something to merge: a collision radius below one pixel (brush 1, stamp radius 0,
# only identical samples collide) and a fine sample step.  08-B keeps its own brush (16 px: bands of radius 8, lines 3 px apart merge into one band).
CFG = dict(collision_radius_intra_px=0.4, hash_stride_px=0.0, dedup_sample_step=3)

# Wp % 64 = 0 / 1 / 63; Hp a multiple of the tile height, and one row more.  The stage itself takes any canvas from 1 x 1 up (its pad and its brush set
# no lower limit), so what bounds the sizes from below is the geometry: the clusters 80 px apart reach x = 185 and y = 128, the bands along the
# borders need room between their ends.  191 / 192 / 193 are the smallest widths >= 186 with the three residues, 192 the smallest height >= 129 whose
# padded height is a multiple of 64, 193 the one after it.
WIDTHS = [192, 193, 191]
HEIGHTS = [192, 193]


def _h(y, x0, x1):
    return [[x0, y], [x1, y]]


def _v(x, y0, y1):
    return [[x, y0], [x, y1]]


def geometries(W, H):
    """{name: polylines} on a W x H canvas (W >= 191, H >= 192)"""
    g = {}
    # three horizontal lines around canvas y = 64 (the band lies across y = 63 | 64 | 65: a tile-row boundary) that cross x = 63 | 64 | 65 (a run that
    # ends on bit 63 next to one that starts on bit 0); alternating directions
    g["horizontal_x64_y64"] = [P(_h(61, 20, 110)), P(_h(64, 112, 22)), P(_h(67, 21, 109))]
    # the same turned: the band lies across the word / tile-column boundary x = 64, every skeleton row links to the row above
    g["vertical_x64_y64"] = [P(_v(61, 20, 110)), P(_v(64, 112, 22)), P(_v(67, 21, 109))]
    # 45 degrees through (64, 64), both ways: where the skeleton steps over the word boundary, the link exists only through the diagonal word
    # neighbour (north-west for the falling diagonal, north-east for the rising one)
    g["diagonal_nw"] = [P([[24, 24], [104, 104]]), P([[108, 104], [28, 24]])]
    g["diagonal_ne"] = [P([[104, 24], [24, 104]]), P([[28, 104], [108, 24]]), P([[100, 24], [20, 104]])]
    # a band long enough that its skeleton fills the whole word of canvas x = 64 .. 127 (and the stamped band several rows of it)
    g["full_word"] = [P(_h(30, 40, 152)), P(_h(33, 150, 42))]
    # along the first and the last canvas column and row (the pad keeps the bands on the raster)
    g["borders"] = [P(_v(0, 30, H - 31)), P(_v(2, H - 31, 30)), P(_v(W - 1, 30, H - 31)), P(_v(W - 3, H - 31, 30)),
                    P(_h(0, 30, W - 31)), P(_h(2, W - 31, 30)), P(_h(H - 1, 30, W - 31)), P(_h(H - 3, W - 31, 30))]
    # two clusters 80 px apart (>= 76: expanded boxes do not overlap), one in each tile of the tile-column boundary x = 64, the right one first in the
    # input and both crossing the tile-row boundary y = 64: group ranks and the component order inside a group both decide the output order
    g["two_clusters"] = [P(_v(140, 20, 120)), P(_v(12, 25, 115)), P(_v(143, 118, 22)), P(_v(15, 113, 27)), P(_h(125, 138, 185)), P(_h(128, 183, 140))]
    return g


def cases():
    """[(id, W, H, polylines)]: every geometry at every width and height"""
    out = []
    for W in WIDTHS:
        for H in HEIGHTS:
            for name, polys in geometries(W, H).items():
                out.append((f"{name}-{W}x{H}", W, H, polys))
    return out


def params(base, W, H, **over):
    """the stage-08 parameter block as {field: value}: `base` (oracle.derived08 zipped with the field names) on a W x H canvas"""
    d = dict(base); d.update(W=W, H=H); d.update(over)
    return d
