"""k_ccl_bits unites runs, not pixels (bitplane.h): its two callers against the oracle on planes made of runs.  Stage 04 (set_edges -> find_contours):
the order of the contour list shows the component labels, so list equality checks them.  Stage 03 (set_masks -> detect_edges): the hysteresis
components decide which candidates are edges.  W runs over one word, its last bit, two words, two words and a bit; the patterns put runs across word
boundaries, runs of the row above that touch a run only at its widened ends, diagonal links only, late merges and long parent chains.  Stage 03 gets
areas (its opening removes one-pixel lines) whose edge rings are such runs, and an all-ones mask in every stack (full words in front of the NMS; a uniform
mask has no candidate, so a full candidate word cannot be made through set_masks -- the full word of the merge pass is stage 04's full row).  The no-GPU
companion shows that the oracle finds several components and several contours in every plane, so that the equalities say something.  On the `stagger`
planes the order of the components by their smallest BLOCK-RASTER pixel id differs from their order by smallest linear id y * W + x (on the other
patterns the two orders agree): the contour list there is in the oracle's order only if the labels are block-raster ids."""
import numpy as np
import pytest

from oracle import oracle as O
from util import same_polys

WS, HS = (8, 63, 64, 65, 129), (8, 9, 33)
SHAPES = [(h, w) for w in WS for h in HS]


# ---------------------------------------------------------------- the patterns: (H, W) -> u8 plane, lines one pixel wide
def rows(H, W):
    """a full row, and below it runs that cross the word boundaries they can reach (x = 63 | 64 and 127 | 128)"""
    e = np.zeros((H, W), np.uint8)
    e[1, :] = 255
    e[4, W // 4:] = 255
    e[H - 2, :max(W // 2, 6)] = 255
    return e


def checker(H, W):
    """diagonal links only; two boards with two empty rows between them"""
    yy, xx = np.mgrid[:H, :W]
    e = (((yy + xx) & 1) == 0).astype(np.uint8) * 255
    e[H // 2 - 1:H // 2 + 1] = 0
    return e


def vlines(H, W):
    e = np.zeros((H, W), np.uint8)
    e[:, ::3] = 255
    return e


def corners(H, W):
    """single pixels in the four corners, and two bars so that there are contours as well"""
    e = np.zeros((H, W), np.uint8)
    e[0, 0] = e[0, W - 1] = e[H - 1, 0] = e[H - 1, W - 1] = 255
    e[2, 1:W - 1] = 255
    e[H - 3, 1:W - 1] = 255
    return e


def comb(H, W):
    """teeth from the top that join only in the last row: every tooth is a component of its own until the merge reaches that row; the spine is cut once"""
    e = np.zeros((H, W), np.uint8)
    e[:, ::2] = 255
    e[H - 1, :] = 255
    c = (W // 2) | 1
    e[:, c - 1:c + 2] = 0
    return e


def spiral(H, W):
    """a one-pixel spiral of pitch 2 over all but the last two columns (a component whose pixels hang on one another in a long line), and a
    line in the last column"""
    e = np.zeros((H, W), np.uint8)
    Wn = W - 2
    free = lambda yy, xx: not (0 <= yy < H and 0 <= xx < Wn and e[yy, xx])
    y = x = 0; dy, dx = 0, 1
    e[0, 0] = 255
    while True:
        for _ in range(2):                                   # straight on while the pixel after the next is free, else one turn to the right
            ny, nx = y + dy, x + dx
            ok = 0 <= ny < H and 0 <= nx < Wn and not e[ny, nx] and free(ny + dy, nx + dx)
            if ok:
                break
            dy, dx = dx, -dy
        if not ok:
            break
        y, x = ny, nx
        e[y, x] = 255
    e[:, W - 1] = 255
    return e


def widened(H, W):
    """a run whose only links to the row above are one pixel at x - 1 of its first and one at x + 1 of its last pixel; at W = 129 these lie in the words
    to the left and to the right of the run's word (x = 63 and 128), at W = 65 the right one does.  Twice, the second copy four rows lower."""
    e = np.zeros((H, W), np.uint8)
    a, b = (64, 127) if W >= 129 else (2, min(W - 2, 63))
    for y in (2, 6):
        e[y, a:b + 1] = 255
        e[y - 2:y, a - 1] = 255
        e[y - 2:y, b + 1] = 255
    return e


def stagger(H, W):
    """vertical lines in every third column, every other one starting a row lower: of two neighbours the one that starts in row 1 lies in the earlier
    2x2 block (smaller block-raster id), the one that starts in row 0 further right has the smaller linear id"""
    e = np.zeros((H, W), np.uint8)
    for i, x in enumerate(range(0, W, 3)):
        e[(i + 1) & 1:, x] = 255
    return e


def ones(H, W):
    return np.full((H, W), 255, np.uint8)


PATTERNS = [rows, checker, vlines, corners, comb, spiral, widened]
STACKS = [(rows, checker, vlines), (corners, comb, spiral), (widened, rows, comb)]          # K = 3, different content per layer


# ---------------------------------------------------------------- masks for stage 03: areas, since the opening takes one-pixel lines away
def wide(H, W):
    """bars three rows high from x = 1 to W - 2: the long sides of their edge rings are runs across every word boundary"""
    e = np.zeros((H, W), np.uint8)
    for y in range(0, H, 6):
        e[y:y + 3, 1:W - 1] = 255
    return e


def diag(H, W):
    """diagonal stripes four pixels wide: edges whose pixels hang together through diagonal links"""
    yy, xx = np.mgrid[:H, :W]
    return ((((xx + yy) // 4) % 2) == 0).astype(np.uint8) * 255


def dots(H, W):
    e = np.zeros((H, W), np.uint8)
    for y in range(0, H - 2, 6):
        for x in range(0, W - 2, 6):
            e[y:y + 3, x:x + 3] = 255
    return e


def bars(H, W):
    e = np.zeros((H, W), np.uint8)
    for x in range(0, W, 8):
        e[:, x:x + 4] = 255
    return e


MASKS = [wide, diag, dots, bars]
MASK_STACKS = [(wide, ones, diag), (dots, bars, ones)]                                       # K = 3; `ones`: full words in front of the NMS, no edge

_cache = {}


def want04(fn, H, W):
    k = ("04", fn.__name__, H, W)
    if k not in _cache:
        e = fn(H, W)
        sk = O.thin_rot(e)
        _cache[k] = (e, sk, [p for p in O.trace(sk) if len(p) >= 5])
    return _cache[k]


def want03(fn, H, W):
    k = ("03", fn.__name__, H, W)
    if k not in _cache:
        m = fn(H, W)
        _cache[k] = (m, O.stage03(m))
    return _cache[k]


# ---------------------------------------------------------------- no GPU: the planes are not trivial
@pytest.mark.parametrize("fn", PATTERNS, ids=lambda f: f.__name__)
def test_oracle_finds_several_components_and_contours(fn):
    for H, W in SHAPES:
        e, sk, polys = want04(fn, H, W)
        n, _ = O.ccl8(sk)                                    # (labels 0 .. n - 1, the background among them)
        assert n - 1 > 1 and len(polys) > 1, (fn.__name__, H, W, n - 1, len(polys))


@pytest.mark.parametrize("fn", MASKS, ids=lambda f: f.__name__)
def test_oracle_finds_several_edge_components(fn):
    for H, W in SHAPES:
        m, ed = want03(fn, H, W)
        n, _ = O.ccl8(ed)
        assert n - 1 > (1 if W >= 63 else 0), (fn.__name__, H, W, n - 1)      # (eight columns hold one dot or bar and its ring of edges)


def component_orders(sk):
    """(labels ordered by their component's smallest block-raster id, by its smallest linear id, the label plane)"""
    _, lab = O.ccl8(sk)
    H, W = sk.shape; Wb = (W + 1) >> 1
    yy, xx = np.nonzero(lab)
    l = lab[yy, xx]
    br = ((((yy >> 1) * Wb + (xx >> 1)) << 2) | ((yy & 1) << 1) | (xx & 1))
    lin = yy * W + xx
    ids = [int(i) for i in np.unique(l)]
    return sorted(ids, key=lambda i: br[l == i].min()), sorted(ids, key=lambda i: lin[l == i].min()), lab


@pytest.mark.parametrize("H,W", SHAPES)
def test_stagger_tells_block_raster_ids_from_linear_ids(H, W):
    """the two orders differ, every component has a contour, and the oracle lists the contours in block-raster order: a CCL that labelled by y * W + x
    would hand stage 04 the same components in another order, and test_stage04_component_order_is_block_raster would see another list"""
    e, sk, polys = want04(stagger, H, W)
    by_block, by_linear, lab = component_orders(sk)
    assert len(by_block) == len(range(0, W, 3)) and by_block != by_linear
    first = [np.asarray(p).reshape(-1, 2)[0] for p in polys]
    assert [int(lab[y, x]) for x, y in first] == by_block


def test_all_ones_mask_has_no_edge():
    """a uniform mask has no gradient, so no candidate can be made of full words through set_masks; the plane still runs as a layer of every stack"""
    assert not O.stage03(ones(9, 65)).any()


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    from orip.device import Device
    d = Device(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
def test_stage04_contours_equal_oracle(dev, H, W):
    from orip.lib import SLOT_CONTOURS
    for stack in STACKS:
        w = [want04(fn, H, W) for fn in stack]
        dev.set_edges(np.stack([x[0] for x in w]))
        dev.find_contours()
        for l, (e, sk, polys) in enumerate(w):
            assert np.array_equal(dev.get_skeleton(l), sk), (stack[l].__name__, H, W, "skeleton")
            got = dev.get_polys(SLOT_CONTOURS, l)
            assert same_polys(got, polys), (stack[l].__name__, H, W, len(got), len(polys))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
def test_stage04_component_order_is_block_raster(dev, H, W):
    """the stagger planes, alone and between two other layers: the contour list in the oracle's order (CPU companion:
    test_stagger_tells_block_raster_ids_from_linear_ids)"""
    from orip.lib import SLOT_CONTOURS
    for stack in [(stagger,), (checker, stagger, rows)]:
        w = [want04(fn, H, W) for fn in stack]
        dev.set_edges(np.stack([x[0] for x in w]))
        dev.find_contours()
        for l, (e, sk, polys) in enumerate(w):
            assert np.array_equal(dev.get_skeleton(l), sk), (stack[l].__name__, H, W, "skeleton")
            got = dev.get_polys(SLOT_CONTOURS, l)
            assert same_polys(got, polys), (stack[l].__name__, H, W, len(got), len(polys))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
def test_stage03_edges_equal_oracle(dev, H, W):
    for stack in MASK_STACKS:
        w = [want03(fn, H, W) for fn in stack]
        dev.set_masks(np.stack([x[0] for x in w]))
        dev.detect_edges()
        for l, (m, ed) in enumerate(w):
            assert np.array_equal(dev.get_edges(l), ed), (stack[l].__name__, H, W)
