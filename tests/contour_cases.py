"""Structured skeletons for stage 04 (csrc/raster04.hip, csrc/walker.h): the inputs on which the device-only paths of the walker run -- chain_jump
(forced stretches of degree-2 pixels, 64 per round), the three row loaders of load_tile, the chain lists and their sizing, the thinning loop and
its cap.  tests/test_oracle_contour_cases.py (CPU) proves on the oracle alone that the maps have the properties they are named after;
tests/test_gpu_contour_cases.py (GPU) compares the device with the oracle on the same maps.  Plain numpy: nothing here touches the oracle or
the device.  Every family is a function returning (names, stack): the members as layers of one uint8 [K,H,W] array, K <= 16."""
import numpy as np

# lengths of the degree-2 chains the closed shapes are built for: around the listing threshold ORIP_CHAIN_MIN = 24, the 64 lanes of a round
# (one, two, three rounds), the "not worth it" rule (8) and 88 = 64 + 24
CHAIN_LENGTHS = [8, 22, 23, 24, 25, 31, 32, 63, 64, 65, 87, 88, 89, 127, 128, 129, 191, 192, 193]
CHAIN_MIN = 24                                  # walker.h: ORIP_CHAIN_MIN
TARGETS = [7, 8, 15, 16, 55, 56, 63, 64]        # the ring of the 64 x 64 window (load_tile puts the cursor in columns 8..55) and the 16-byte rounding of tx0
WIDTHS = [256, 260, 257, 263]                   # W % 16 == 0: 16-byte rows; W % 4 == 0 only: 4-byte words; odd: bytes
PLACE_H = 256

_N8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


# ---------------------------------------------------------------- what a skeleton is made of (used by both test modules, on the ORACLE's skeleton)
def degrees(sk):
    """number of 8-neighbours of every skeleton pixel (0 off the skeleton)"""
    fg = np.asarray(sk) > 0
    H, W = fg.shape
    p = np.pad(fg, 1).astype(np.int32)
    deg = sum(p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in _N8)
    return deg * fg


def chains(sk):
    """the maximal chains of degree-2 pixels, as k_chain_ends_bits / k_chain_build see them: a degree-2 pixel with a skeleton neighbour that is
    not degree-2 is a chain end; from an end the chain follows the degree-2 neighbour that is not the pixel before.  Returns a list of
    (pixels, has_end): pixels [(y, x), ...] in chain order; has_end False for a ring of degree-2 pixels (no end, never listed)."""
    fg = np.asarray(sk) > 0
    H, W = fg.shape
    d2 = fg & (degrees(sk) == 2)

    def nbs(y, x, m):
        return [(y + dy, x + dx) for dy, dx in _N8 if 0 <= y + dy < H and 0 <= x + dx < W and m[y + dy, x + dx]]

    is_end = np.zeros_like(d2)
    for y, x in zip(*np.nonzero(d2)):
        is_end[y, x] = any(not d2[q] for q in nbs(y, x, fg))
    seen = np.zeros_like(d2)
    out = []
    for start_set, has_end in ((is_end, True), (d2, False)):
        for y, x in zip(*np.nonzero(start_set)):
            if seen[y, x]:
                continue
            pix = [(int(y), int(x))]; seen[y, x] = True
            while True:
                nx = [q for q in nbs(*pix[-1], d2) if not seen[q]]
                if not nx:
                    break
                seen[nx[0]] = True; pix.append((int(nx[0][0]), int(nx[0][1])))
            out.append((pix, has_end))
    return out


def listed_lengths(sk):
    """lengths of the chains the device lists: with an end, at least CHAIN_MIN long"""
    return sorted(len(p) for p, e in chains(sk) if e and len(p) >= CHAIN_MIN)


# ---------------------------------------------------------------- drawing
def _line(e, p, q):
    (y0, x0), (y1, x1) = p, q
    n = max(abs(y1 - y0), abs(x1 - x0))
    for i in range(n + 1):
        e[y0 + (y1 - y0) * i // max(n, 1), x0 + (x1 - x0) * i // max(n, 1)] = 255


def _rect(e, y0, x0, h, w):
    e[y0, x0:x0 + w] = 255; e[y0 + h - 1, x0:x0 + w] = 255; e[y0:y0 + h, x0] = 255; e[y0:y0 + h, x0 + w - 1] = 255


def _put(canvas, shape, y0, x0):
    h, w = shape.shape
    assert 0 <= y0 and 0 <= x0 and y0 + h <= canvas.shape[0] and x0 + w <= canvas.shape[1], (canvas.shape, shape.shape, y0, x0)
    assert not canvas[max(y0 - 2, 0):y0 + h + 2, max(x0 - 2, 0):x0 + w + 2].any(), "members may not touch"
    canvas[y0:y0 + h, x0:x0 + w] = shape


def _stack(maps, H, W, at=(3, 3)):
    """small shapes -> layers of one [K,H,W] array, each put at `at`"""
    out = np.zeros((len(maps), H, W), np.uint8)
    for k, m in enumerate(maps):
        _put(out[k], m, *at)
    return out


# ---------------------------------------------------------------- closed shapes: no endpoint, every path comes from a leftover walk
THETA_H = 9


def theta(n, transposed=False):
    """a (n + 4) x 9 rectangle outline with a middle bar: thins to three degree-2 chains of exactly n pixels (top, bar, bottom; the sides are
    a few pixels each) and no endpoint.  Tight: the chains' left ends lie at column 2, rows 0, 4 and 8."""
    e = np.zeros((THETA_H, n + 4), np.uint8)
    _rect(e, 0, 0, THETA_H, n + 4)
    e[THETA_H // 2, :] = 255
    return e.T.copy() if transposed else e


def diamond(r, chord=True, flat=0, transposed=False):
    """four diagonals (steps +-(W +- 1)) of radius r, optionally with the horizontal chord between the side corners.  flat = 1 doubles the
    centre column (a two-pixel apex), which makes the chain lengths even.  The raster-first pixel is the apex: a degree-2 pixel inside a chain."""
    S = 2 * r + 1
    e = np.zeros((S, S + flat), np.uint8)
    for sx, ox in ((-1, 0), (1, flat)):
        _line(e, (0, r + ox), (r, r + ox + sx * r)); _line(e, (2 * r, r + ox), (r, r + ox + sx * r))
    if flat:
        e[0, r:r + 2] = 255; e[2 * r, r:r + 2] = 255
    if chord:
        e[r, :] = 255
    return e.T.copy() if transposed else e


def thetas(transposed, part):
    """one theta per layer, chain lengths CHAIN_LENGTHS[:10] (part 0) or [10:] (part 1); upright (steps +-1) or transposed (steps +-W)"""
    ls = CHAIN_LENGTHS[:10] if part == 0 else CHAIN_LENGTHS[10:]
    maps = [theta(n, transposed) for n in ls]
    H, W = (208, 16) if transposed else (16, 208)
    return [f"theta{'T' if transposed else ''}_{n}" for n in ls], _stack(maps, H, W)


# (radius, flat): chains of 2r - 3 + flat (the two halves) and 2r - 5 + flat (the chord) pixels
DIAMONDS = [(12, 0), (13, 0), (13, 1), (14, 0), (14, 1), (15, 0), (33, 0), (33, 1), (34, 0), (34, 1), (35, 0), (40, 0), (66, 0)]
RING_R = 40                                     # the chordless diamond: a ring of 160 degree-2 pixels


def diamonds():
    maps = [diamond(r, True, f) for r, f in DIAMONDS] + [diamond(RING_R, False)]
    names = [f"diamond_r{r}_f{f}" for r, f in DIAMONDS] + ["diamond_ring"]
    return names, _stack(maps, 140, 144)


def _ring(e, y0, x0, h, w, square):
    """rectangle outline; not square: without its corner pixels, so a turn is a diagonal step between two degree-2 pixels and a chain runs round it
    (a square corner keeps three mutually adjacent pixels after thinning, a junction)"""
    _rect(e, y0, x0, h, w)
    if not square:
        for y, x in ((y0, x0), (y0, x0 + w - 1), (y0 + h - 1, x0), (y0 + h - 1, x0 + w - 1)):
            e[y, x] = 0


def figure_eight(h, w, square=False):
    """two rectangle loops that meet in one corner"""
    e = np.zeros((2 * h - 1, 2 * w - 1), np.uint8)
    _ring(e, 0, 0, h, w, square); _ring(e, h - 1, w - 1, h, w, square)
    e[h - 1, w - 1] = 255
    return e


def nested(h, w, gap, bridges, square=False):
    """two concentric rectangles joined by one or two straight bridges"""
    e = np.zeros((h, w), np.uint8)
    _ring(e, 0, 0, h, w, square); _ring(e, gap, gap, h - 2 * gap, w - 2 * gap, square)
    e[h // 2, 0:gap + 1] = 255
    if bridges > 1:
        e[h - gap - 1:h, w // 3] = 255
    return e


def loops():
    """chains that turn corners inside a round, and leftover walks that start mid-chain and leave a chain partly visited for the next walk
    (names ending in _sq: square corners, straight chains between junction clusters)"""
    maps = [figure_eight(20, 30, True), figure_eight(20, 30), figure_eight(40, 70), figure_eight(70, 40), figure_eight(90, 120),
            nested(60, 80, 6, 1, True), nested(60, 80, 6, 1), nested(60, 80, 6, 2), nested(150, 200, 10, 1), nested(150, 200, 10, 2), nested(200, 150, 25, 2),
            nested(150, 200, 10, 2, True), np.pad(diamond(30), ((0, 0), (0, 59)))]
    d = maps[-1]; d[:, 60:] = diamond(30)[:, 1:]                  # two diamonds sharing a side corner
    names = ["eight_20x30_sq", "eight_20x30", "eight_40x70", "eight_70x40", "eight_90x120", "nested_60x80_1_sq", "nested_60x80_1", "nested_60x80_2",
             "nested_150x200_1", "nested_150x200_2", "nested_200x150_2", "nested_150x200_2_sq", "diamond_pair"]
    return names, _stack(maps, 248, 246)


# ---------------------------------------------------------------- placement: the members with chains of 64 and 129 against the borders, the window ring
# and the column rounding, in images of every loader's width class
D64 = (33, 1)       # diamond(33, flat=1): halves of 64
D129 = (66, 0)      # diamond(66): halves of 129
# offset of a chain end inside the tight shape, (dy, dx): the left end of the theta's top chain; the end next to the left (upright) / top
# (transposed) corner of a diamond's upper-left diagonal.  tests/test_oracle_contour_cases.py proves the ends land where they are aimed.
THETA_END = (0, 2)


def _diamond_end(r):
    return (r - 2, 2)


def place_thetas(W):
    """layers 0..3: theta 64 with the left end of its top chain at (t, t) and theta 129 at (t + 128, t), t = TARGETS[i] and TARGETS[i + 4] in one
    layer; layers 4..7: the same transposed (129 at (t, t + 128)); layers 8, 9: 64 and 129 touching row 0, row H-1, column 0 and column W-1"""
    H = PLACE_H
    out = np.zeros((10, H, W), np.uint8); names = []
    for tr in (False, True):
        for i in range(4):
            l = i + (4 if tr else 0)
            for t in (TARGETS[i], TARGETS[i + 4]):
                for n, far in ((64, 0), (129, 128)):
                    y, x = t - THETA_END[0], t - THETA_END[1]
                    if tr:
                        _put(out[l], theta(n, True), x, y + far)
                    else:
                        _put(out[l], theta(n), y + far, x)
            names.append(f"theta{'T' if tr else ''}_at_{TARGETS[i]}_{TARGETS[i + 4]}")
    for l, n in ((8, 64), (9, 129)):
        s = theta(n); w = n + 4
        _put(out[l], s, 0, 90); _put(out[l], s, H - THETA_H, 60)
        _put(out[l], s.T.copy(), 40, 0); _put(out[l], s.T.copy(), 60, W - THETA_H)
        names.append(f"theta_{n}_borders")
    return names, out


def place_diamonds(W, which):
    """which = 64: layer i has diamond 64 upright with its upper-left chain end at x = TARGETS[i] and transposed with it at y = TARGETS[i]; layers
    8, 9: an apex on row 0, row H-1 (upright) and column 0, column W-1 (transposed), layer 10: one further than 64 px from every border.
    which = 129: layers 0..7 upright, 8..15 transposed (two of 133 px do not fit one layer side by side with the targets)."""
    H = PLACE_H
    r, f = D64 if which == 64 else D129
    up, tr = diamond(r, True, f), diamond(r, True, f, transposed=True)
    ey, ex = _diamond_end(r)
    S = 2 * r + 1
    if which == 64:
        out = np.zeros((11, H, W), np.uint8); names = []
        for i, t in enumerate(TARGETS):
            _put(out[i], up, H - S - 20, t - ex)
            _put(out[i], tr, t - ex, W - S - 24)
            names.append(f"diamond64_at_{t}")
        _put(out[8], up, 0, 0); _put(out[8], up, H - S, W - S - f)
        _put(out[9], tr, 0, 0); _put(out[9], tr, H - S - f, W - S)         # (thinning takes the tip off a side corner: columns 0 and W-1 are touched by an apex)
        _put(out[10], up, 94, 94)
        return names + ["diamond64_corners_a", "diamond64_corners_b", "diamond64_centre"], out
    out = np.zeros((16, H, W), np.uint8); names = []
    for i, t in enumerate(TARGETS):
        _put(out[i], up, (H - S, 0, 61, 100)[i % 4], t - ex)
        _put(out[8 + i], tr, t - ex, (W - S, 0, 61, 100)[i % 4])
        names += [f"diamond129_x_{t}"]
    names += [f"diamond129T_y_{t}" for t in TARGETS]
    return names, out


# ---------------------------------------------------------------- open long paths: endpoint walks, the compiled stepping, the window re-placed in all directions
def _polyline(e, verts, chamfer=True):
    """straight runs between the vertices; chamfer clears the inner vertices, so that a right-angle turn is a diagonal step between two degree-2
    pixels (a square corner keeps three mutually adjacent pixels after thinning: a junction at every turn)"""
    for p, q in zip(verts[:-1], verts[1:]):
        _line(e, p, q)
    if chamfer:
        for y, x in verts[1:-1]:
            e[y, x] = 0


def spiral(n, pitch=4, close=False):
    """rectangular spiral of n turns inwards, arms `pitch` px apart, corners chamfered: one open path of degree-2 pixels.  close joins the inner
    end to the neighbouring arm: one junction and one endpoint, so the leftover walk that follows the endpoint walk covers chains of several
    hundred pixels with corners."""
    S = 2 * n * pitch + 8
    e = np.zeros((S, S), np.uint8)
    lo, hi = 2, S - 3
    verts = [(lo, lo)]
    for _ in range(n):
        verts += [(lo, hi), (hi, hi), (hi, lo), (lo + pitch, lo)]
        lo += pitch; hi -= pitch
    verts[-1] = (verts[-1][0], verts[-1][1])
    if close:
        verts.append((lo - pitch, lo))                           # up onto the arm the last turn started from
    else:
        verts.append((lo, lo + pitch))
    _polyline(e, verts)
    if close:
        e[lo - pitch, lo] = 255
    return e


def serpentine(H, W, pitch=6):
    e = np.zeros((H, W), np.uint8)
    verts = []
    for i, y in enumerate(range(2, H - 2, pitch)):
        verts += [(y, 2), (y, W - 3)] if i % 2 == 0 else [(y, W - 3), (y, 2)]
    _polyline(e, verts)
    return e


def zigzag(H, W, amp=20, rows=4):
    """45-degree zigzags, one above the other, alternately starting upwards and downwards"""
    e = np.zeros((H, W), np.uint8)
    for k in range(rows):
        y0 = 4 + k * (amp + 8); x = 3; up = k % 2 == 1
        while x + amp < W - 3:
            a, b = (y0 + amp, y0) if up else (y0, y0 + amp)
            _line(e, (a, x), (b, x + amp)); x += amp; up = not up
    return e


LINE_LENGTHS = (63, 64, 65, 300)


def straight_lines(anti):
    """separate lines of LINE_LENGTHS px.  anti False: horizontal (step +1), vertical (+W) and down-right (+W + 1); anti True: up-right (-W + 1:
    two diagonals of 300 px in one map would cross)"""
    e = np.zeros((320, 320), np.uint8)
    for i, n in enumerate(LINE_LENGTHS):
        if anti:
            y0, x0 = ((70, 3), (110, 40), (150, 80), (319, 20))[i]
            _line(e, (y0, x0), (y0 - n + 1, x0 + n - 1))
        else:
            e[2 + 3 * i, 14:14 + n] = 255
            e[16:16 + n, 2 + 3 * i] = 255
            y0, x0 = ((20, 60), (20, 130), (20, 200), (20, 20))[i]
            _line(e, (y0, x0), (y0 + n - 1, x0 + n - 1))
    return e


def open_paths():
    S = 320
    sp, spc = spiral(13, 4), spiral(13, 4, close=True)          # about 3,000 pixels
    maps = [sp, spc, sp.T.copy(), spc[::-1, ::-1].copy(), serpentine(124, 310), serpentine(124, 310).T.copy(), zigzag(120, 314), zigzag(120, 314).T.copy(), straight_lines(False), straight_lines(True)]
    names = ["spiral", "spiral_closed", "spiral_T", "spiral_closed_rot", "serpentine", "serpentine_T", "zigzag", "zigzag_T", "lines", "lines_anti"]
    return names, _stack(maps, S + 2, S + 3, at=(1, 1))


LONG_OPEN = ("spiral", "spiral_closed", "spiral_T", "spiral_closed_rot", "serpentine", "serpentine_T")     # the window must be re-placed: tiles > walks


# ---------------------------------------------------------------- many small things
def comb(W=300):
    e = np.zeros((50, W), np.uint8)
    e[45, 2:W - 2] = 255
    for i, x in enumerate(range(4, W - 4, 4)):
        n = 3 + i % 4
        if i % 17 == 5:
            n = 30 + i % 11
        e[45 - n:45, x] = 255
    return e


def ladder(H=200, W=12, every=3):
    e = np.zeros((H, W), np.uint8)
    e[:, 0] = 255; e[:, W - 1] = 255
    e[::every, :] = 255
    return e


def specks(H=200, W=200, seed=404):
    """isolated pixels and strokes of 2..4 pixels on a grid of 6 px: every path is below the 5-point filter, the component count is large"""
    rng = np.random.default_rng(seed)
    e = np.zeros((H, W), np.uint8)
    for y in range(2, H - 6, 6):
        for x in range(2, W - 6, 6):
            n = int(rng.integers(1, 5)); dy, dx = [(0, 1), (1, 0), (1, 1), (1, -1)][int(rng.integers(0, 4))]
            for i in range(n):
                e[y + dy * i, x + 3 + dx * i] = 255
    return e


def small_things():
    sp = specks()
    sp[100:100 + 7, 100:100 + 40] = 0; sp[103, 102:138] = 255      # one line among the specks: the layer keeps a path
    maps = [comb(), comb().T.copy(), ladder(), ladder().T.copy(), ladder(120, 40, 5), sp]
    return ["comb", "comb_T", "ladder", "ladder_T", "ladder_wide", "specks"], _stack(maps, 306, 306)


# ---------------------------------------------------------------- narrow images: W = 1, 2, 3
NARROW_H = 200


def narrow(W):
    H = NARROW_H
    full = np.full((H, W), 255, np.uint8)
    col = np.zeros((H, W), np.uint8); col[3:H - 5, 0] = 255
    maps, names = [full, col], ["full", "column"]
    if W >= 2:
        tri = lambda t: (W - 1) - np.abs(t % (2 * (W - 1)) - (W - 1))                                  # 0 .. W-1 .. 0: one column per step
        zz = np.zeros((H, W), np.uint8); zz[np.arange(H), tri(np.arange(H))] = 255
        z3 = np.zeros((H, W), np.uint8); z3[np.arange(H), tri(np.arange(H) // 3)] = 255                 # runs of three, then the next column
        gaps = full.copy(); gaps[::37] = 0; gaps[5::41, 0] = 0
        maps += [zz, z3, gaps]; names += ["zigzag", "zigzag3", "full_gaps"]
        # a chain between two junction clusters (a row with both border columns set where the path changes sides): the endpoint walks stop on the
        # first junction pixel, so only a leftover walk visits the chain.  In two columns the zigzag's steps are +W + 1 and +W - 1 = +1.
        for kind in ("zigzag", "column"):
            e = np.zeros((H, W), np.uint8)
            e[0:5, 0] = 255; e[4, :] = 255
            ys = np.arange(5, 160); e[ys, tri(ys) if kind == "zigzag" else W - 1] = 255
            e[160, :] = 255; e[160:190, 0] = 255
            maps.append(e); names.append(kind + "_junctions")
    if W == 3:
        lad = np.zeros((H, W), np.uint8); lad[:, 0] = 255; lad[:, 2] = 255; lad[::30, :] = 255; lad[H - 1, :] = 255
        maps.append(lad); names.append("ladder30")          # vertical chains >= 24 between the rungs, no endpoint
    return names, np.stack(maps)


# ---------------------------------------------------------------- thick shapes: the thinning loop (two iterations per host round trip, cap 120)
SMALL_SQUARES = [2, 3, 4, 5, 6, 7, 9, 12]
THIN_CAP = 120                                   # raster04.hip: `for (int it = 0; it < 120; it += 2)`


def _filled(n, S):
    """a filled n x n square at (2, 2) of an S x S map, and a stroke of 12 px below it: a filled square or disc thins to a single pixel, which is
    no path, and every map must keep one (the stroke is thin already: the square alone decides how many iterations the loop runs)"""
    e = np.zeros((S, S), np.uint8); e[2:2 + n, 2:2 + n] = 255
    e[S - 3, 3:15] = 255
    return e


def small_squares():
    """end after 1 .. 6 deleting iterations: both parities of the loop's exit test (it asks after every second iteration)"""
    return [f"square_{n}" for n in SMALL_SQUARES], np.stack([_filled(n, 20) for n in SMALL_SQUARES])


def thick():
    S = 320
    disc = _filled(0, S); yy, xx = np.mgrid[:S, :S]; disc[(yy - 150) ** 2 + (xx - 150) ** 2 <= 60 * 60] = 255
    bar = np.zeros((S, S), np.uint8); bar[3:303, 100:140] = 255
    maps = [disc, _filled(250, S), _filled(300, S), bar, bar.T.copy()]
    return ["disc_60", "square_250", "square_300", "bar_300x40", "bar_40x300"], np.stack(maps)


# ---------------------------------------------------------------- the capacity pair
# raster04.hip, orip_contours_prepare ("forced stretches"): with M the skeleton pixel count of the context's PREVIOUS prepare,
#     m_guess = M + M / 4 + 4096;  cap_ends = m_guess;  cap_cpix = 2 * m_guess + 256
# chain ends beyond cap_ends and chains whose m + 2 entries do not fit cap_cpix are not listed.  `crowded` after `small` must exceed BOTH
# limits twice over (a condition, not a measurement: the case survives a modest retuning of the sizing).
def cap_ends_after(M):
    return M + M // 4 + 4096


def cap_cpix_after(M):
    return 2 * cap_ends_after(M) + 256


def capacity_small():
    e = np.zeros((1, 256, 256), np.uint8); e[0, 100, 100:110] = 255
    return ["small"], e


def capacity_crowded():
    """8 layers of 256 x 256 tiled with 68 x 9 thetas (three chains of 64 each, a few short ones at the sides: about twenty chain ends per
    theta), and 38 x 9 ones in the strip that is left"""
    e = np.zeros((8, 256, 256), np.uint8)
    for l in range(8):
        for y in range(1 + l % 3, 256 - 10, 11):
            for x in (1, 72, 143):
                e[l, y:y + THETA_H, x:x + 68] = theta(64)
            e[l, y:y + THETA_H, 214:214 + 38] = theta(34)
    return [f"crowded_{l}" for l in range(8)], e


# name -> builder of (names, stack); the GPU module runs every one under every switch
FAMILIES = {
    "theta_a": lambda: thetas(False, 0), "theta_b": lambda: thetas(False, 1), "thetaT_a": lambda: thetas(True, 0), "thetaT_b": lambda: thetas(True, 1),
    "diamonds": diamonds, "loops": loops,
    **{f"place_theta_{W}": (lambda W=W: place_thetas(W)) for W in WIDTHS},
    **{f"place_d64_{W}": (lambda W=W: place_diamonds(W, 64)) for W in WIDTHS},
    **{f"place_d129_{W}": (lambda W=W: place_diamonds(W, 129)) for W in WIDTHS},
    "open": open_paths, "small_things": small_things,
    "narrow1": lambda: narrow(1), "narrow2": lambda: narrow(2), "narrow3": lambda: narrow(3),
    "small_squares": small_squares, "thick": thick,
}
CLOSED = ["theta_a", "theta_b", "thetaT_a", "thetaT_b", "diamonds", "loops"]      # no member has a degree-1 pixel
