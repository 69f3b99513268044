"""Sequences of stage 08-B calls for ONE device context, each call finding the group canvas as the calls before it left it: 08-B no longer clears
the canvas (vector08b.hip, B08::gid), so a call's result may depend on nothing but the pixels it stamped itself.  tests/test_oracle_stale_canvas_cases.py
(CPU) shows with the oracle's raster that on every call stale stamps lie against the new band and, at brush 1, against the new skeleton;
tests/test_gpu_stage08b_stale_canvas.py (GPU) compares every call with the oracle.  Plain data and numpy: nothing here touches the oracle or the device.

Canvas sizes and the 08-A settings (which leave near-parallel lines to 08-B) are those of tests/skel_merge_cases.py: padded widths = 0, 1, 63 (mod 64)."""
import numpy as np

import skel_merge_cases as C
from skel_merge_cases import P, _h, _v

CFG = C.CFG
WIDTHS = C.WIDTHS
H1, H2 = C.HEIGHTS            # 192 for the sequence, 193 on the canvas of the other width
BRUSHES = [16, 1]             # post_brush at its default (stamp radius 8) and at 1 (radius 0: the band IS the lines, the skeleton lies on its border)

# the skel_merge_cases geometries in an order in which the band of each lies across or against the band of the one before
MERGE_ORDER = ["horizontal_x64_y64", "vertical_x64_y64", "diagonal_nw", "diagonal_ne", "full_word", "two_clusters", "borders"]


def spacing(brush):
    """distance of near-parallel lines whose bands merge: 3 px under the 16-px brush (skel_merge_cases), 1 px under the 1-px brush (8-adjacent rows)"""
    return 3 if brush >= 8 else 1


def own_geometries(W, H, brush):
    """{name: polylines}: a lone line gives 08-B nothing to merge, so every 'line' is a pair `spacing` apart, drawn in opposite directions"""
    s, rad = spacing(brush), max(1, brush) // 2
    g = {}
    # a thick bundle: eight lines from the left border to the right one (178+ px: a box row spans three and four words), one wide band
    g["bundle"] = [P(_h(60 + s * i, 0, W - 1) if i % 2 == 0 else _h(60 + s * i, W - 1, 0)) for i in range(8)]
    # thin, through the middle of that band: every pixel it stamps was stamped before, with stale stamps on both sides
    g["thin"] = [P(_h(60 + 3 * s, 30, 150)), P(_h(60 + 4 * s, 150, 30))]
    # beside: its band ends on the row above the bundle's band (60 - rad is the bundle's first row)
    yb = 59 - 2 * rad - s
    g["beside"] = [P(_h(yb, 20, 160)), P(_h(yb + s, 160, 20))]
    # vertical, from the top border to the bottom one, across all of the above
    g["vertical"] = [P(_v(100, 0, H - 1)), P(_v(100 + s, H - 1, 0))]
    # diagonal, across the bundle and the vertical pair
    g["diagonal"] = [P([[20, 20], [150, 150]]), P([[150 + s, 150], [20 + s, 20]])]
    # along all four borders, against the ends of the bundle and of the vertical pair
    g["borders"] = [P(_v(0, 30, H - 31)), P(_v(s, H - 31, 30)), P(_v(W - 1, 30, H - 31)), P(_v(W - 1 - s, H - 31, 30)),
                    P(_h(0, 30, W - 31)), P(_h(s, W - 31, 30)), P(_h(H - 1, 30, W - 31)), P(_h(H - 1 - s, W - 31, 30))]
    return g


def sequence(W, brush):
    """[(name, W, H, polylines)] in call order, for one context: the own geometries, under the default brush the skel_merge_cases geometries, then the
    bundle on a canvas of another width (the stale values land at other pixels) and the thin pair back on the first one"""
    g = own_geometries(W, H1, brush)
    seq = [(n, W, H1, g[n]) for n in ("bundle", "thin", "beside", "vertical", "diagonal", "borders")]
    if brush >= 8:
        m = C.geometries(W, H1)
        seq += [("merge_" + n, W, H1, m[n]) for n in MERGE_ORDER]
    W2 = WIDTHS[(WIDTHS.index(W) + 1) % len(WIDTHS)]
    seq.append(("bundle_other_width", W2, H2, own_geometries(W2, H2, brush)["bundle"]))
    seq.append(("thin_back", W, H1, g["thin"]))
    return seq
