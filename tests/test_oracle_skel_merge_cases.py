"""The stage 08-B cases of tests/skel_merge_cases.py deserve the name: on every one the oracle's stage-08 result with the skeleton merge differs from the
one without it and holds at least one merged line, so the equality tests/test_gpu_skel_merge_cases.py asserts says something about 08-B.  CPU only."""
import numpy as np
import pytest

from oracle import oracle as O
import skel_merge_cases as C
from util import same_polys

_FIELDS08 = ["tap_diam", "tap_max_dim", "min_keep", "tap_max_per", "tap_max_v", "sample_step", "tail_len_px", "col_rad", "grid_stride", "max_jump",
             "post_on", "post_brush", "post_step", "post_eps", "post_minlen", "W", "H", "brush_forbid"]
_BASE = dict(zip(_FIELDS08, O.derived08(dict(O.DEFAULTS, **C.CFG))))


def _run(W, H, polys, **over):
    d = C.params(_BASE, W, H, **over)
    return O.stage08_layer(polys, np.array([d[k] for k in _FIELDS08], np.float64))


def test_the_padded_sizes_are_what_they_say():
    assert sorted((W + 128) % 64 for W in C.WIDTHS) == [0, 1, 63]
    assert [(H + 128) % 64 for H in C.HEIGHTS] == [0, 1]
    assert max(C.WIDTHS + C.HEIGHTS) + 128 <= 400
    assert len(C.cases()) == len(C.WIDTHS) * len(C.HEIGHTS) * 7
    # the sizes are the smallest with these residues that hold the geometry: it reaches x = 185 and y = 128 on every canvas
    for _, W, H, polys in C.cases():
        q = np.concatenate([np.asarray(p).reshape(-1, 2) for p in polys])
        assert q.min() >= 0 and q[:, 0].max() < W and q[:, 1].max() < H
    q = np.concatenate([np.asarray(p).reshape(-1, 2) for p in C.geometries(191, 192)["two_clusters"]])
    assert q[:, 0].max() == 185 and q[:, 1].max() == 128
    assert min(C.WIDTHS) - 64 < 186 and min(C.HEIGHTS) - 64 < 129


@pytest.mark.parametrize("name,W,H,polys", C.cases(), ids=[c[0] for c in C.cases()])
def test_skeleton_merge_changes_the_result(name, W, H, polys):
    on_l, on_t = _run(W, H, polys)
    off_l, off_t = _run(W, H, polys, post_on=0)
    assert len(off_l) == len(polys), "stage 08-A must hand every line to 08-B"
    assert len(on_l) >= 1
    assert len(on_l) < len(off_l), "near-parallel lines merge"
    assert not same_polys(on_l, off_l)
    for p in on_l:          # inside the canvas: the skeleton of a band along a border stays on it
        q = np.asarray(p).reshape(-1, 2)
        assert q[:, 0].min() >= 0 and q[:, 0].max() < W and q[:, 1].min() >= 0 and q[:, 1].max() < H


def test_two_clusters_come_out_in_group_order():
    """the right cluster is first in the input, so its merged lines come first in 08-B's list (before the travel reorder): both clusters are there"""
    for W in C.WIDTHS:
        on_l, _ = _run(W, 192, C.geometries(W, 192)["two_clusters"])
        xs = sorted(float(np.asarray(p).reshape(-1, 2)[:, 0].mean()) for p in on_l)
        assert xs[0] < 64 and xs[-1] > 128, xs
