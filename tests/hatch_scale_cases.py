"""TEST INFRASTRUCTURE: named inputs that drive the capped grid-stride loops of the fill (csrc/fill.hip: k_fl_sample, k_fl_scatter), the stipple
(csrc/gcode_stipple.hip: k_st_test, k_st_emit) and the hatch link (csrc/gcode_link.hip: k_hl_elig) into a second and a third pass, the stipple's occlusion
into its second and third batch of 64 shapes, and the hatch link's pointer jumping over a chain of 2 500 lines.  tests/test_hatch_scale_host.py shows with
the counting functions below and the doubles alone that every case reaches what it is named after; tests/test_gpu_hatch_scale.py runs them on the device
against the doubles, by equality.  No GPU import, no test here.

The constants restate the kernels' launch geometry.  The host test counts the units of every case from them, so a change of a cap that is mirrored here makes
the case names fail instead of silently no longer reaching a second pass; a change that is not mirrored is caught by test_constants_are_the_kernels, which
reads them out of the sources.

A UNIT is what one wave takes at a time: a block of 64 samples of a hatch line (fill), a chunk of 64 lattice slots of a shape (stipple), a pair
(END a, START b) in reach (hatch link)."""
import functools

import numpy as np

import fill_cases as FC
import fill_double as FD
import hatch_double as HD
import hatch_link_cases as LC
import stipple_cases as SC
import stipple_double as SD

FL_BLOCKS = 16384                  # k_fl_sample, k_fl_scatter: min(FL_BLOCKS, cdiv(Z, FL_WAVES)) blocks of FL_WAVES waves, a wave per block of samples
FL_WAVES = 4
ST_BLOCKS = 8192                   # k_st_test, k_st_emit: min(ST_BLOCKS, C) blocks of one wave, a wave per chunk
HL_BLOCKS = 16384                  # k_hl_elig: min(HL_BLOCKS, P) blocks of one wave, a wave per pair
BATCH = 64                         # k_st_test takes the shapes above 64 at a time


def passes(units, cap, waves=1):
    """rounds of a grid-stride loop over `units` whose grid is min(cap, cdiv(units, waves)) blocks of `waves` waves"""
    if units == 0:
        return 0
    grid = min(cap, -(-units // waves)) * waves
    return -(-units // grid)


# ================================================================================================ fill
def fill_families(c):
    """the families of a fill as the host of orip_fill_mask lays them out (include/orip.h states the frame; the head of fill.hip the lines and blocks):
    -> [{"u", "NW", "kmin", "L", "blocks", "first"}], `first` the family's first block"""
    W, H, (ux, uy) = c["W"], c["H"], c["u"]
    out, z = [], 0
    for (fx, fy), bit in (((ux, uy), FC.ALONG), ((-uy, ux), FC.ACROSS)):
        if not c["flags"] & bit:
            continue
        _, D, m, _, _ = FD.frame((fx, fy), c["spacing"], 0, 1)
        NW = ((W if abs(fx) >= abs(fy) else H) + 63) // 64
        cx, cy = -fy * (W - 1), fx * (H - 1)                                             # n.p at the corners: 0, cx, cy, cx + cy
        lo, hi = min(0, cx) + min(0, cy), max(0, cx) + max(0, cy)
        kmin = -((-(lo - m)) // D)
        L = max(0, (hi + m) // D - kmin + 1)
        out.append(dict(u=(fx, fy), NW=NW, kmin=kmin, L=L, blocks=L * NW, first=z))
        z += L * NW
    return out


def fill_units(c):
    return sum(f["blocks"] for f in fill_families(c))


def random_mask(h, w, seed, p=0.6):
    return ((np.random.RandomState(seed).rand(h, w) < p) * 255).astype(np.uint8)


ROWS = dict(u=(4096, 0), spacing=2)                                                      # line k is the canvas row y = 2 k: L = H // 2 + 1 lines
# name: (blocks, passes).  The first pass of four-wave blocks ends at 4 FL_BLOCKS = 65 536 blocks.
FILL_UNITS = {
    "rows_cap": (65536, 1),                                                              # 65 536 lines of one block
    "rows_cap_plus_1": (65537, 2),                                                       # one wave makes a second pass
    "rows_two_passes": (98307, 2),                                                       # 32 769 lines of 3 blocks
    "rows_and_columns": (165891, 3),                                                     # and 66 columns of 1 024 blocks, from block 98 307 on
    "rows_and_columns_serpentine": (165891, 3),
    "oblique_tall": (69536, 2),                                                          # 17 384 lines of 4 blocks
    "oblique_tall_negative_u": (69536, 2),
}
CLOSED_FORM = ("rows_cap", "rows_cap_plus_1", "rows_two_passes")                         # fill_cases.rows_closed_form applies


@functools.lru_cache(maxsize=None)
def fill_cases():
    """Every mask is a seeded random one.  At W = 130 under (64, 1, -200, 0) mask column 3 is a = 0 .. 55, column 4 a = 56 .. 119 and column 5 a = 120 .. 129:
    runs cross a = 63 / 64 and 127 / 128 and are cut by both canvas edges.  At W = 256 under (7, 2, -45, -33) a mask pixel is 3.5 canvas pixels."""
    C = {}
    thin = random_mask(32772, 20, 1)                                                     # 4 canvas pixels a mask pixel, from x = -6: a = 0 .. 63 is cut at both ends
    C["rows_cap"] = FC.case(thin, 64, 131070, (4, 1, -6, -3), inset=1, min_len=4, flags=FC.ALONG, **ROWS)
    C["rows_cap_plus_1"] = FC.case(thin, 64, 131072, (4, 1, -6, -3), inset=1, min_len=4, flags=FC.ALONG, **ROWS)
    wide = random_mask(1024, 6, 2)
    two = dict(W=130, H=65536, place=(64, 1, -200, 0), inset=1, min_len=2, **ROWS)
    C["rows_two_passes"] = FC.case(wide, flags=FC.SERPENTINE | FC.ALONG, **two)
    C["rows_and_columns"] = FC.case(wide, flags=FC.ALONG | FC.ACROSS, **two)
    C["rows_and_columns_serpentine"] = FC.case(wide, flags=FC.SERPENTINE | FC.ALONG | FC.ACROSS, **two)
    tall = random_mask(11440, 90, 3)
    for name, u in (("oblique_tall", (3547, 2048)), ("oblique_tall_negative_u", (-3547, 2048))):
        C[name] = FC.case(tall, 256, 40000, (7, 2, -45, -33), u, 2, inset=2, min_len=5, flags=FC.SERPENTINE | FC.ALONG)
    assert set(C) == set(FILL_UNITS)
    return C


# ================================================================================================ stipple
def stipple_shapes(c):
    """the shapes of a stipple case, ascending, as k_st_plan plans them: -> [{"group", "box", "j0", "nrows", "cols", "slots", "chunks"}]; a shape without an
    edge of positive length has no slot"""
    p, q, _ = c["lattice"]
    off, pts = np.asarray(c["ring_off"]).tolist(), np.asarray(c["ring_pts"], np.int64).reshape(-1, 2)
    shapes = {}
    for r, g in enumerate(np.asarray(c["ring_group"]).tolist()):
        P = pts[off[r]:off[r + 1]]
        s = shapes.setdefault(g, dict(group=g, box=None, has=False))
        b = (int(P[:, 0].min()), int(P[:, 1].min()), int(P[:, 0].max()), int(P[:, 1].max()))
        s["box"] = b if s["box"] is None else (min(b[0], s["box"][0]), min(b[1], s["box"][1]), max(b[2], s["box"][2]), max(b[3], s["box"][3]))
        s["has"] = s["has"] or bool((P != np.roll(P, -1, 0)).any())
    out = []
    for g in sorted(shapes):
        s = shapes[g]
        x0, y0, x1, y1 = s["box"]
        j0 = -((-y0) // q)
        nrows, cols = (max(0, y1 // q - j0 + 1), (x1 - x0) // p + 1) if s["has"] else (0, 0)
        out.append(dict(s, j0=j0, nrows=nrows, cols=cols, slots=nrows * cols, chunks=-(-(nrows * cols) // 64)))
    return out


def stipple_units(c):
    return sum(s["chunks"] for s in stipple_shapes(c))


def slot_points(c, shape):
    """the slots of one shape of stipple_shapes(c), ascending: -> (x, y, is a lattice point of the box), the way the head of gcode_stipple.hip numbers them"""
    p, q, sft = c["lattice"]
    k = np.arange(shape["slots"], dtype=np.int64)
    j = shape["j0"] + k // shape["cols"]
    sh = np.where(j & 1, sft, 0)
    x = (-((-(shape["box"][0] - sh)) // p) + k % shape["cols"]) * p + sh
    return x, j * q, x <= shape["box"][2]


def batch_of(c, below, above):
    """the batch of 64 in which the shape of group `below` meets the shape of group `above`: 0 is the first"""
    groups = sorted(set(np.asarray(c["ring_group"]).tolist()))
    return (groups.index(above) - groups.index(below) - 1) // BATCH


def decoy(i):
    """small squares far from the 1000-step square: no chunk of it meets one"""
    x, y = 100 + 150 * (i % 30), 2000 + 150 * (i // 30)
    return SC.rect_ring(x, y, x + 100, y + 100)


def unit_squares(count):
    """squares 100 wide, 100 in a row: 3 or 4 lattice rows of 3 columns each, one chunk a shape"""
    return [SC.rect_ring(x, y, x + 100, y + 100) for x, y in ((100 + 110 * (k % 100), 100 + 110 * (k // 100)) for k in range(count))]


COVER = SC.rect_ring(400, 300, 900, 800)                                                 # over the middle of the 1000-step square
COVER_AT = {1: 64, 2: 65, 3: 129}                                                        # hidden_by_batch_N: the shape that hides, of 140
STRIPS = [SC.rect_ring(130 + 200 * i, 50, 230 + 200 * i, 1150) for i in range(5)]         # five strips down the whole square
HALF_A, HALF_B = SC.rect_ring(50, 50, 1150, 610), SC.rect_ring(50, 400, 1150, 1150)      # first_batch_hides_all: shape 1 and shape 70
# name: (chunks, passes).  The first pass of one-wave blocks ends at ST_BLOCKS = 8 192 chunks.
STIPPLE_UNITS = {
    "one_shape_two_passes": (8556, 2),                                                   # 521 rows of 1 051 columns: 547 571 slots
    "squares_12000": (10887, 2),                                                         # of 12 000 shapes; 1 113 hold no slot
    "chunks_cap": (8192, 1),
    "chunks_cap_plus_1": (8193, 2),
    "hidden_by_batch_1": (152, 1), "hidden_by_batch_2": (152, 1), "hidden_by_batch_3": (152, 1),
    "hidden_by_the_second_batch_only": (85, 1),
    "first_batch_hides_all": (95, 1),
}


@functools.lru_cache(maxsize=None)
def stipple_cases():
    C = {}
    # serpentine with an odd shift: an odd row takes its places from the row's other end, and with 8 192 chunks between a wave's two chunks the masks and
    # scan words it reads there were written by other waves in the other pass
    C["one_shape_two_passes"] = SC.case([SC.rect_ring(100, 100, 2200, 620)], [0], lattice=(2, 1, 1), inset=3, flags=SD.SERPENTINE)
    C["squares_12000"] = SC.case(SC.many_squares(12000, per_row=100), list(range(12000)), inset=5, rect=(0, 0, 12000, 14000))
    for name, n in (("chunks_cap", ST_BLOCKS), ("chunks_cap_plus_1", ST_BLOCKS + 1)):
        C[name] = SC.case(unit_squares(n), list(range(n)), inset=5, rect=(0, 0, 12000, 14000), flags=SD.SERPENTINE)
    for k, at in COVER_AT.items():
        C[f"hidden_by_batch_{k}"] = SC.case([SC.SQUARE] + [COVER if i == at else decoy(i) for i in range(1, 140)], list(range(140)), flags=SD.OCCLUDE | SD.SERPENTINE)
    C["hidden_by_the_second_batch_only"] = SC.case([SC.SQUARE] + [decoy(i) for i in range(1, 65)] + STRIPS, list(range(70)), flags=SD.OCCLUDE | SD.SERPENTINE)
    C["first_batch_hides_all"] = SC.case([SC.SQUARE, HALF_A] + [decoy(i) for i in range(2, 70)] + [HALF_B], list(range(71)), flags=SD.OCCLUDE | SD.SERPENTINE)
    assert set(C) == set(STIPPLE_UNITS)
    return C


def without(c, group):
    """a stipple case with the rings of one group taken out"""
    keep = np.nonzero(np.asarray(c["ring_group"]) != group)[0]
    off = np.asarray(c["ring_off"]).tolist()
    return SC.case([[tuple(q) for q in c["ring_pts"][off[r]:off[r + 1]].tolist()] for r in keep], c["ring_group"][keep], c["lattice"], c["inset"], c["rect"], c["flags"])


# ================================================================================================ hatch link
def link_lines(c):
    """-> (START int64 [nl, 2], END int64 [nl, 2], class [nl]) of the lines: the strokes of exactly two points with a class"""
    off, pts, cls = np.asarray(c["off"], np.int64), np.asarray(c["pts"], np.int64).reshape(-1, 2), np.asarray(c["cls"], np.int64)
    ln = np.nonzero((np.diff(off) == 2) & (cls >= 0))[0]
    return pts[off[ln]], pts[off[ln] + 1], cls[ln]


def link_units(c):
    """the pairs (END a, START b) in reach, from the rule alone: a < b, one class, |dx|, |dy| <= reach and dx^2 + dy^2 <= reach^2"""
    S, E, cls = link_lines(c)
    n, reach = len(S), int(c["reach"])
    d = S[None, :, :] - E[:, None, :]
    ok = (np.arange(n)[None, :] > np.arange(n)[:, None]) & (cls[None, :] == cls[:, None]) & (np.abs(d) <= reach).all(2) & ((d * d).sum(2) <= reach * reach)
    return int(ok.sum())


def jump_rounds(nl):
    """the rounds of pointer jumping the host fixes: the least R with 2^R >= nl"""
    r = 0
    while (1 << r) < nl:
        r += 1
    return r


def dense(n, seed=3):
    """n lines of one class with both ends on a grid of 4 steps in the patch (100, 100) - (200, 200), under a star polygon that holds a part of the patch:
    every END reaches every later START, a good share of the pairs leaves or touches the star, and on 26 x 26 grid points distances tie all the time"""
    rng = np.random.default_rng(seed)
    ring = [tuple(p) for p in HD.star(rng, 150, 150, 90, 9).tolist()]
    strokes = []
    while len(strokes) < n:
        a, b = (100 + 4 * rng.integers(0, 26, 2)).tolist(), (100 + 4 * rng.integers(0, 26, 2)).tolist()
        if a != b:
            strokes.append([tuple(a), tuple(b)])
    return LC.case(strokes, [0] * n, [ring], [0], reach=200)


TALL_U = [(x + 100, y + 100) for x, y in [(0, 0), (440, 0), (440, 50000), (240, 50000), (240, 200), (200, 200), (200, 50000), (0, 50000)]]
# name: (lines, pairs in reach, passes, jump rounds).  The first pass of one-wave blocks ends at HL_BLOCKS = 16 384 pairs.
LINK_UNITS = {
    "dense_181": (181, 16290, 1, 8),
    "dense_182": (182, 16471, 2, 8),
    "dense_200": (200, 19900, 2, 8),
    "tall_rectangle": (2500, 22455, 2, 12),                                              # one chain of 2 500 lines: 12 rounds, none to spare
    "tall_u": (2495, 39756, 3, 12),                                                      # two legs 40 apart: the pairs across the gap meet the ring
}


@functools.lru_cache(maxsize=None)
def link_cases():
    C = {f"dense_{n}": dense(n) for n in (181, 182, 200)}
    C["tall_rectangle"] = LC.hatched([[SC.rect_ring(100, 100, 300, 100100)]], reach=400)
    C["tall_u"] = LC.hatched([[TALL_U]], reach=400)
    assert set(C) == set(LINK_UNITS)
    return C


# the case with the most data of every pass, and the small case of the existing files that runs directly behind it
LARGEST = {"fill": "rows_and_columns_serpentine", "stipple": "one_shape_two_passes", "link": "tall_u"}
SMALL = {"fill": "rect_hole_p0_u3", "stipple": "square", "link": "square"}
