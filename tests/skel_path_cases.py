"""Deterministic inputs for the path search of stage 08-B (csrc/vector08b.hip: component order, anchors, the chunked FIFO search, resample, RDP, the three
size classes) and for its four parameters away from their defaults: post_brush, post_step, post_eps, post_minlen, which no config key reaches.
tests/test_oracle_skel_path_cases.py (CPU) shows on the oracle alone that every case is what its name says; tests/test_gpu_skel_path_cases.py (GPU)
compares the device with the oracle.  Plain data and numpy: nothing here touches the oracle or the device.

A case is (id, W, H, polylines, overrides of orip_params08 fields, ORIP_COMP_CAPS or None).  Stage 08-A is made transparent with skel_merge_cases.CFG.
The defaults are post_brush 16, post_step 6, post_eps 1.28, post_minlen 32; groups that are meant to be separate lie at least 4 brush + 12 px apart."""
import numpy as np

from skel_merge_cases import P, CFG, geometries as merge_geometries          # noqa: F401  (CFG is part of this module's interface)


def L(x0, y0, x1, y1):
    return P([[x0, y0], [x1, y1]])


def pair(x0, y0, x1, y1, dx=0, dy=3):
    """a line and its antiparallel twin, offset by (dx, dy): one band at every brush from 4 up"""
    return [L(x0, y0, x1, y1), L(x1 + dx, y1 + dy, x0 + dx, y0 + dy)]


def brush_fields(b):
    """post_eps and post_minlen as the reference derives them from the brush (08:504-505)"""
    return dict(post_brush=b, post_eps=max(1.0, 0.08 * b), post_minlen=max(2 * b, 12))


# ---------------------------------------------------------------- path choice
TIE = pair(20, 100, 120, 100)                                  # both 100 long: the longest line is the one with the lower index


def circle(cx, cy, r, n, phase=0.0):
    """one closed polyline (first == last) of n segments"""
    return P([[cx + round(r * np.cos(2 * np.pi * k / n + phase)), cy + round(r * np.sin(2 * np.pi * k / n + phase))] for k in range(n + 1)])


RING = [circle(100, 100, 80, 40)]         # 08-A drops the closing samples: the ends map to skeleton pixels a few apart, the anchored path is short, the diameter runs on a cycle
HAIRPIN = [P([[100, 100], [250, 100], [100, 102]])]            # both ends of the longest line map to ONE skeleton pixel (a0 == a1)
LOLLIPOP = [P([[60, 100], [260, 100], [60, 102]]), circle(300, 100, 40, 24, np.pi)]      # a0 == a1 at the tip of the stick, the diameter search runs over the ring
OUT_AND_BACK = [P([[100, 100], [250, 100], [110, 103]])]       # both ends of the longest line lie near x = 100: the anchored path is short
OUT_AND_BACK_TAIL = OUT_AND_BACK + [L(250, 101, 400, 101)]     # the diameter leaves the longest line's own band
ANCHORS_OUTSIDE = [L(100, 100, 300, 100), L(120, 141, 280, 140)]      # one group, two components: the second holds no anchor
NESTED = [L(100, 100, 100, 500), L(100, 500, 500, 500), L(103, 500, 103, 100)] + pair(300, 200, 400, 200)      # the pair lies in the hollow of the L's ROI
# the same with the L in 100-px pieces and a longer pair: stage 08-A hands its lines over longest first, so the pair's group gets the lower rank
NESTED_PIECES = ([L(100, y, 100, y + 100) for y in (100, 200, 300, 400)] + [L(x, 500, x + 100, 500) for x in (100, 200, 300, 400)]
                 + [L(103, y + 100, 103, y) for y in (400, 300, 200, 100)] + pair(300, 200, 420, 200))
X_CROSS = [L(100, 100, 300, 300), L(300, 100, 100, 300)]
HASH = [L(100, 150, 300, 150), L(300, 250, 100, 250), L(150, 100, 150, 300), L(250, 300, 250, 100)]
COMB = [L(50, 250, 350, 250)] + [L(x, 250, x, 150) for x in (80, 140, 200, 260, 320)]
SHORT = [L(100, 100, 130, 100)]                                # 30 px: below post_minlen at the defaults, and at most one large step long
OBLIQUE = [L(30, 30, 150, 90), L(152, 94, 32, 34)]


def order_case(dx, dy, control=False):
    """A (left) and B (right) in one group, two components whose merged lines are both 96 long: the travel reorder at the end of stage 08 starts at the
    longest line, the FIRST of the two, so the component order decides the output.  B's pixels start a row above A's, but in the same row of 2 x 2
    blocks counted from the ROI's first row (an odd canvas row), so A, further left, comes first; a key from canvas coordinates puts B first in all
    four.  control: A two rows lower, B comes first."""
    if control:
        return [L(100, 103, 200, 103), L(250, 101, 353, 101)]
    return [L(100 + dx, 100 + dy, 200 + dx, 100 + dy), L(250, 99, 353, 99)]


LINE300 = [L(50, 100, 350, 100)]


def band300(y=100):
    return pair(50, y, 350, y)


def hband(n, x0=40, y=100):
    """a horizontal band whose lines are n px long"""
    return pair(x0, y, x0 + n, y)


DIAG_E = 760                                                   # the 45-degree band (20, 20) -> (760, 760): a skeleton of about 725 px
DIAG = pair(20, 20, DIAG_E, DIAG_E, 2, -2)
OBLIQUE_LONG = pair(20, 20, 380, 740, 3, -1)                    # slope 2: diagonal and straight steps alternate, every pixel a corner, 1.2 px of length per pixel
# two shorter staircases 390 px apart in one group: two components, each with more resample points (and, at tolerance 0, more kept points) than pixels,
# so every per-component offset that scales with the points per pixel is taken at a component base other than 0
STAIRS2 = pair(20, 20, 340, 660, 3, -1) + pair(410, 20, 730, 660, 3, -1)
DIAG_SMALL = pair(24, 24, 168, 168, 2, -2)

# band lengths whose skeleton component has S % 8 == 0 and S % 8 == 1 pixels (the CPU companion asserts both): the class boundaries S == cap, S == cap + 1
BAND_S8 = 137
BAND_S9 = 139
S8 = 128
S9 = 129


def random_walks(seed, n=20, size=400):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(3, 9))
        p = np.empty((k, 2), np.int64); p[0] = rng.integers(30, size - 30, 2)
        for i in range(1, k):
            p[i] = np.clip(p[i - 1] + rng.integers(-70, 71, 2), 8, size - 9)
        out.append(P(p))
    return out


def combo(seed):
    rng = np.random.default_rng(1000 + seed)
    return dict(post_brush=int(rng.integers(2, 41)), post_step=float(np.round(rng.uniform(1.0, 9.0), 3)), post_eps=float(np.round(rng.uniform(0.0, 3.0), 3)),
                post_minlen=int(rng.integers(0, 60)))


# ids whose result is, by a stated identity, the default result on the same input (asserted as an equality by the CPU companion); every other case
# with overrides must differ from the default result
SAME_AS_DEFAULT = set()


def cases():
    c = []

    def add(name, W, H, polys, over=None, caps=None, same=False):
        c.append((name, W, H, polys, dict(over or {}), caps))
        if same:
            SAME_AS_DEFAULT.add(name)

    # ---- path choice, at the defaults
    add("tie_first", 192, 192, TIE)
    add("tie_second", 192, 192, TIE[::-1])
    add("ring", 208, 208, RING)
    add("hairpin", 272, 192, HAIRPIN)
    add("lollipop", 400, 192, LOLLIPOP)
    add("out_and_back", 272, 192, OUT_AND_BACK)
    add("out_and_back_tail", 416, 192, OUT_AND_BACK_TAIL)
    add("anchors_outside", 320, 192, ANCHORS_OUTSIDE)
    for dy in (0, 1):
        for dx in (0, 1):
            add(f"order_dx{dx}_dy{dy}", 384, 192, order_case(dx, dy))
    add("order_control", 384, 192, order_case(0, 0, control=True))
    add("nested_L_first", 528, 528, NESTED)
    add("nested_pair_first", 528, 528, NESTED_PIECES)
    add("x_cross", 320, 320, X_CROSS)
    add("hash", 320, 320, HASH)
    add("comb", 400, 272, COMB)
    # ---- size classes: (8, 65000) puts every component above 8 px into the large LDS class, (8, 8) into global scratch; no hook: the small one
    for name, W, H, polys in (("ring", 208, 208, RING), ("lollipop", 400, 192, LOLLIPOP), ("hash", 320, 320, HASH), ("comb", 400, 272, COMB), ("band", 400, 208, band300())):
        if name == "band":
            add("band-small", W, H, polys)
        add(f"{name}-large", W, H, polys, caps="8,65000")
        add(f"{name}-global", W, H, polys, caps="8,8")
    add("band_S8-cap0_eq", 192, 192, hband(BAND_S8), caps=f"{S8},{S8 + 8}")         # S == cap0: small class
    add("band_S9-cap0_plus1", 192, 192, hband(BAND_S9), caps=f"{S9 - 1},{S9 + 7}")   # S == cap0 + 1: large class
    add("band_S8-cap1_eq", 192, 192, hband(BAND_S8), caps=f"8,{S8}")                 # S == cap1: large class
    add("band_S9-cap1_plus1", 192, 192, hband(BAND_S9), caps=f"8,{S9 - 1}")          # S == cap1 + 1: global
    # ---- post_brush
    for b in (-2, 0, 1, 2, 3):               # (below 1 the stamp radius stays max(1, b) / 2 = 0 and only the boxes' growth 2 b + 6 shrinks: accepted, as the reference does)
        add(f"brush{b}", 192, 192, TIE + OBLIQUE, brush_fields(b))
    # the band of ONE 300-px line: 2 (brush / 2) + 1 px thick, thinned from both sides in about brush / 4 iterations
    for b in (26, 40, 60, 100, 128):
        add(f"brush{b}-line", 400, 208, LINE300, brush_fields(b))              # 100 and 128: thinning stops at its cap of 48 on an unfinished, fat component
    add("brush100-line-large", 400, 208, LINE300, brush_fields(100), caps="8,65000")      # the fat component (small class by itself) in the other two
    add("brush100-line-global", 400, 208, LINE300, brush_fields(100), caps="8,8")
    for b in (40, 60):
        for g in ("horizontal_x64_y64", "vertical_x64_y64"):
            # (the 90-px lines leave a path of 75 .. 78 px, below the derived post_minlen of 80 / 120, which would hide the skeleton: the default 32)
            add(f"brush{b}-{g}", 192, 192, merge_geometries(192, 192)[g], dict(brush_fields(b), post_minlen=32))
    add("brush128-borders", 528, 528, [L(0, 100, 0, 500), L(100, 0, 500, 0)], brush_fields(128))      # bands that end on the raster's first column and row
    add("brush129-borders", 528, 528, [L(0, 100, 0, 500), L(2, 500, 2, 100), L(527, 500, 527, 100)], brush_fields(129))      # the widest accepted: radius 64 = the pad
    # ---- post_step
    for s in (1.0, 1.2):
        add(f"step{s}-diag", 800, 800, DIAG, dict(post_step=s))
        add(f"step{s}-diag-600", 800, 800, DIAG, dict(post_step=s), caps="8,600")
        add(f"step{s}-diag-global", 800, 800, DIAG, dict(post_step=s), caps="8,8")
    for s in (1.5, 2.5):
        add(f"step{s}-diag_small", 192, 192, DIAG_SMALL, dict(post_step=s))
        add(f"step{s}-ring", 208, 208, RING, dict(post_step=s))
    add("step50-short", 192, 192, SHORT, dict(post_step=50.0, post_minlen=2))          # total <= step: the path's pixels pass through
    add("step4000-short", 192, 192, SHORT, dict(post_step=4000.0, post_minlen=2))
    add("step4000-band", 400, 208, band300(), dict(post_step=4000.0))                   # 299 pixels pass through, more than the small class had room for
    add("step4000-band-large", 400, 208, band300(), dict(post_step=4000.0), caps="8,65000")
    add("step4000-band-global", 400, 208, band300(), dict(post_step=4000.0), caps="8,8")
    add("step1e300-band", 400, 208, band300(), dict(post_step=1e300))
    # ---- post_eps
    add("eps0.05-ring", 208, 208, RING, dict(post_eps=0.05))
    add("eps0.05-step1-diag", 800, 800, DIAG, dict(post_eps=0.05, post_step=1.0))
    add("eps0.05-step1-ring-global", 208, 208, RING, dict(post_eps=0.05, post_step=1.0), caps="8,8")
    add("eps0-step1-oblique", 400, 800, OBLIQUE_LONG, dict(post_eps=0.0, post_step=1.0))
    add("eps0-step1-oblique-global", 400, 800, OBLIQUE_LONG, dict(post_eps=0.0, post_step=1.0), caps="8,8")
    add("eps0-step1-stairs2-small", 800, 688, STAIRS2, dict(post_eps=0.0, post_step=1.0))
    add("eps0-step1-stairs2-large", 800, 688, STAIRS2, dict(post_eps=0.0, post_step=1.0), caps="8,65000")
    add("eps0-step1-stairs2-global", 800, 688, STAIRS2, dict(post_eps=0.0, post_step=1.0), caps="8,8")
    add("eps0-ring", 208, 208, RING, dict(post_eps=0.0))
    add("eps1e9-ring_comb", 400, 480, RING + [P(np.asarray(p).reshape(-1, 2) + [0, 200]) for p in COMB], dict(post_eps=1e9))
    # ---- post_minlen (need = max(2, post_minlen))
    for m in (2, 0, -5):
        add(f"minlen{m}", 400, 400, COMB + [L(100, 20, 130, 20)], dict(post_minlen=m))
    add("minlen_eq_path", 192, 192, TIE, dict(post_minlen=TIE_PATH), same=True)
    add("minlen_path_plus1", 192, 192, TIE, dict(post_minlen=TIE_PATH + 1))
    add("minlen500", 400, 272, COMB, dict(post_minlen=500))
    # ---- all four at once
    for seed in range(3):
        add(f"combo{seed}", 400, 400, random_walks(seed), combo(seed))
    return c


TIE_PATH = 92              # pixels of the anchored path of TIE at the defaults (the CPU companion asserts it against O.component_best_path)

# refusals: (overrides, message)
REFUSALS = [(dict(post_step=0.999), r"postmerge_resample_step must be >= 1"),
            (dict(post_step=float("nan")), r"postmerge_resample_step must be >= 1"),
            (dict(post_brush=130), r"postmerge brush 130 out of range: at most 129"),
            (dict(post_brush=100000), r"postmerge brush 100000 out of range: at most 129")]
