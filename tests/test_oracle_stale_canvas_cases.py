"""The sequences of tests/stale_canvas_cases.py deserve the name.  With numpy and the oracle's own raster (stamp_capsule, zs_std) on the padded canvas, a
model of the canvas memory is carried from call to call -- stage 08-B never clears it, so what lies there is the union of ALL earlier stamps, re-read
row by row when the canvas width changes -- and for every call after the first of a sequence:
  * stamps of earlier calls that this call does not restamp lie on the border of this call's band (8-adjacent to a pixel it stamps): a dense pass that
    took them for foreground would widen the band;
  * under brush 1, where the band is the lines themselves, they lie 8-adjacent to this call's SKELETON: exactly where k_nbr_build looks;
  * the call merges something: its result with the skeleton merge differs from the one without and has fewer lines.
CPU only."""
import numpy as np
import pytest

from oracle import oracle as O
import skel_merge_cases as C
import stale_canvas_cases as SC
from util import same_polys

PAD = 64                                       # vector08b.hip: PAD8
_FIELDS08 = ["tap_diam", "tap_max_dim", "min_keep", "tap_max_per", "tap_max_v", "sample_step", "tail_len_px", "col_rad", "grid_stride", "max_jump",
             "post_on", "post_brush", "post_step", "post_eps", "post_minlen", "W", "H", "brush_forbid"]
_BASE = dict(zip(_FIELDS08, O.derived08(dict(O.DEFAULTS, **SC.CFG))))


def _run(W, H, polys, **over):
    d = C.params(_BASE, W, H, **over)
    return O.stage08_layer(polys, np.array([d[k] for k in _FIELDS08], np.float64))


def _stamp(W, H, lines, brush):
    """the band 08-B stamps for `lines` (what 08-A hands over) on the padded canvas, as 0 / 1 bytes"""
    m = np.zeros((H + 2 * PAD, W + 2 * PAD), np.uint8)
    for p in lines:
        q = np.asarray(p).reshape(-1, 2) + PAD
        for (x0, y0), (x1, y1) in zip(q[:-1], q[1:]):
            O.stamp_capsule(m, x0, y0, x1, y1, max(1, brush) // 2)
    return (m > 0).astype(np.uint8)


def _dilate8(a):
    p = np.pad(a, 1)
    h, w = a.shape
    return np.max([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)


@pytest.mark.parametrize("brush", SC.BRUSHES)
@pytest.mark.parametrize("W", SC.WIDTHS)
def test_stale_stamps_lie_against_every_later_call(W, brush):
    seq = SC.sequence(W, brush)
    names = [s[0] for s in seq]
    assert names[:3] == ["bundle", "thin", "beside"] and names[-2:] == ["bundle_other_width", "thin_back"]
    assert seq[-2][1] != W and seq[-1][1] == W and ("merge_two_clusters" in names) == (brush >= 8)
    mem = np.zeros(0, np.uint8)                # the canvas memory, flat: 1 where some earlier call stamped
    for i, (name, w, h, polys) in enumerate(seq):
        on_l, _ = _run(w, h, polys, post_brush=brush)
        off_l, _ = _run(w, h, polys, post_brush=brush, post_on=0)
        assert len(off_l) == len(polys), (name, "stage 08-A must hand every line to 08-B")
        assert 1 <= len(on_l) < len(off_l) and not same_polys(on_l, off_l), (name, "near-parallel lines merge")
        band = _stamp(w, h, off_l, brush)
        Hp, Wp = band.shape
        old = np.zeros(Hp * Wp, np.uint8)
        n = min(len(mem), Hp * Wp); old[:n] = mem[:n]
        old = old.reshape(Hp, Wp)
        if i > 0:
            stale = (old > 0) & (band == 0)
            assert stale.any(), name
            assert (stale & (_dilate8(band) > 0)).any(), (name, "no stale stamp on the border of the band")
            if brush == 1:
                sk = (O.zs_std(band * 255) > 0).astype(np.uint8)
                assert (stale & (_dilate8(sk) > 0)).any(), (name, "no stale stamp next to the skeleton")
        if name == "thin":                      # through the MIDDLE of the bundle's band: it was stamped before (but for a pixel here and there that 08-A's
            # resampling moved), with stale stamps on both sides
            ys = np.nonzero(band.any(axis=1))[0]
            assert old[band > 0].mean() >= 0.95 and old[ys[0] - 1].any() and old[ys[-1] + 1].any()
        if name == "beside":                    # beside the old band, not on it (08-A's resampling moves a sample by a pixel here and there: a handful of
            # pixels may be shared), and against it along its whole length of 140 px
            assert int(((old > 0) & (band > 0)).sum()) <= 8 and int((stale & (_dilate8(band) > 0)).sum()) >= 100
        new = np.maximum(old, band).ravel()
        mem = np.concatenate([new, mem[len(new):]])


def test_the_sequences_hold_what_the_kernels_need():
    for brush in SC.BRUSHES:
        for W in SC.WIDTHS:
            g = SC.own_geometries(W, SC.H1, brush)
            q = np.concatenate([np.asarray(p).reshape(-1, 2) for ps in g.values() for p in ps])
            assert q[:, 0].min() == 0 and q[:, 1].min() == 0 and q[:, 0].max() == W - 1 and q[:, 1].max() == SC.H1 - 1      # all four canvas borders
            assert q.min() >= 0
            spans = [np.ptp(np.asarray(p).reshape(-1, 2), axis=0) for ps in g.values() for p in ps]
            assert any(dx > 128 and dy == 0 for dx, dy in spans)          # a box row of three words and more
            assert any(dx == 0 and dy > 64 for dx, dy in spans)           # vertical
            assert any(dx == dy and dx > 64 for dx, dy in spans)          # diagonal
    assert sorted((W + 2 * PAD) % 64 for W in SC.WIDTHS) == [0, 1, 63]
