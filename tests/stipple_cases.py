"""TEST INFRASTRUCTURE: the named drawings of --stipple-mm (include/orip.h: orip_gcode_stipple), shapes in steps.  Unless a case says otherwise: lattice
(40, 40, 0), inset 27, the rect (0, 0, 6000, 6000), no flags.  A case is a dict of the seven arguments of stipple_double.stipple / Device.gcode_stipple:
ring_off, ring_pts, ring_group, lattice, inset, rect, flags."""
import numpy as np

from hatch_link_cases import SQUARE, L_SHAPE, U_SHAPE, SLIT, ngon
import stipple_double as SD

TOP = 1 << 30
RECT = (0, 0, 6000, 6000)


def case(rings, ring_group, lattice=(40, 40, 0), inset=27, rect=RECT, flags=0):
    """rings as lists of point lists"""
    r_off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    r_pts = np.asarray([q for r in rings for q in r], np.int32).reshape(-1, 2)
    return dict(ring_off=r_off, ring_pts=r_pts, ring_group=np.asarray(ring_group, np.int32).reshape(-1), lattice=tuple(lattice), inset=int(inset), rect=tuple(rect), flags=int(flags))


def rect_ring(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def comb(teeth=40):
    """a comb of `teeth` teeth 30 wide, 20 apart, from y = 300 to y = 900 on a back from y = 100: a row through the teeth crosses 2 * teeth edges"""
    right = 100 + 50 * (teeth - 1) + 30
    pts = [(100, 100), (right, 100)]
    for k in reversed(range(teeth)):
        x0 = 100 + 50 * k
        pts += [(x0 + 30, 900), (x0, 900)]
        if k:
            pts += [(x0, 300), (x0 - 20, 300)]
    return pts


def many_squares(count=300, seed=5, per_row=20):
    """small squares side by side, 10 .. 90 wide: some narrower than the pitch, some between two rows, so that groups without a dot stand among the others"""
    rng = np.random.default_rng(seed)
    rings = []
    for k in range(count):
        x, y, w, h = 100 + 110 * (k % per_row), 100 + 110 * (k // per_row), int(rng.integers(10, 91)), int(rng.integers(10, 91))
        rings.append(rect_ring(x, y, x + w, y + h))
    return rings


def near_diagonal(inset):
    """a sliver three lattice steps wide along an edge of slope 1 + 3 / 2^27 at 2^29: cross(d, w) is k 2^47 + 3 wx, its square passes 2^94, and for the
    lattice points of the first diagonal beside the edge cross^2 >= inset^2 L turns on the 3 wx"""
    a, w, p = 1 << 29, 1 << 27, 1 << 20
    return case([[(a, a), (a + w, a + w + 3), (a + w, a + w - 3 * p)]], [0], lattice=(p, p, 0), inset=inset, rect=(0, 0, TOP, TOP))


def cases():
    C = {}
    C["square"] = case([SQUARE], [0])
    C["square_stagger"] = case([SQUARE], [0], lattice=(40, 35, 20), flags=SD.SERPENTINE)
    C["l_shape"] = case([L_SHAPE], [0], flags=SD.SERPENTINE)
    C["u_shape"] = case([U_SHAPE], [0])
    C["slit"] = case([SLIT], [0])
    C["gon_100"] = case([ngon(600, 600, 500, 100)], [0], flags=SD.SERPENTINE)
    C["ring_with_hole"] = case([ngon(1000, 1000, 1000, 48), ngon(1000, 1000, 400, 24)], [0, 0])
    C["comb_40_teeth"] = case([comb()], [0], lattice=(20, 40, 10), inset=5, flags=SD.SERPENTINE)
    C["many_squares"] = case(many_squares(), list(range(300)), inset=5)
    C["big_square_fine_pitch"] = case([SQUARE], [0], lattice=(10, 10, 0), flags=SD.SERPENTINE)
    two = [SQUARE, rect_ring(600, 600, 1600, 1600)]
    three = two + [ngon(1100, 600, 400, 12)]
    for name, rings in (("overlap_2", two), ("overlap_3", three)):
        C[name] = case(rings, [3, 7, 900000000][:len(rings)], flags=SD.SERPENTINE)
        C[name + "_occlude"] = case(rings, [3, 7, 900000000][:len(rings)], flags=SD.SERPENTINE | SD.OCCLUDE)
    C["hole_on_top_occlude"] = case([SQUARE, rect_ring(300, 300, 900, 900), rect_ring(500, 500, 700, 700)], [0, 1, 1], flags=SD.OCCLUDE)      # the upper shape's hole hides nothing
    C["half_off_sheet"] = case([SQUARE], [0], rect=(0, 0, 600, 4000))
    C["negative_rows"] = case([[(x - 3000, y - 3000) for x, y in L_SHAPE]], [0], lattice=(40, 35, 20), rect=(-4000, -4000, -1, -1), flags=SD.SERPENTINE)
    C["inset_0_vertex_on_lattice"] = case([rect_ring(80, 80, 400, 400)], [0], inset=0)
    C["edge_on_row"] = case([[(0, 0), (400, 0), (400, 240), (200, 240), (0, 440)]], [0], inset=0)      # a horizontal edge on the row y = 240, a diagonal through lattice points
    C["ray_through_vertex"] = case([[(200, 0), (400, 200), (200, 400), (0, 200)]], [0], inset=0)
    C["ray_through_vertex_inset"] = case([[(200, 0), (400, 200), (200, 400), (0, 200)]], [0], inset=29)      # the first diagonal inside is 40 / sqrt 2 = 28.3 away
    C["zero_length_edges"] = case([[(100, 100), (100, 100), (1100, 100), (1100, 1100), (1100, 1100), (1100, 1100), (100, 1100), (100, 100)]], [0])
    C["ring_of_one_point"] = case([[(500, 500)], SQUARE, [(2000, 2000)]], [0, 1, 1])
    C["no_rings"] = case([], [])
    C["pitch_larger_than_shape"] = case([rect_ring(100, 100, 130, 130), rect_ring(121, 121, 159, 159), rect_ring(300, 100, 700, 110)], [0, 1, 2], inset=5)
    C["near_diagonal_a"] = near_diagonal(741456)                          # every lattice point of the first diagonal that the other edge leaves is clear: 43 dots,
    C["near_diagonal_b"] = near_diagonal(741457)                          # 18 of them, the far ones, whose 3 wx is large enough,
    C["near_diagonal_c"] = near_diagonal(741458)                          # none
    # a band across the whole coordinate range, eight rows high under the top: differences of 2^31, the largest pitch, row and inset
    C["far_corners"] = case([rect_ring(-TOP, TOP - (8 << 20), TOP, TOP)], [0], lattice=(1 << 20, 1 << 20, 1 << 19), inset=1 << 20, rect=(-TOP, -TOP, TOP, TOP), flags=SD.SERPENTINE)
    return C


def args(c):
    return c["ring_off"], c["ring_pts"], c["ring_group"], c["lattice"], c["inset"], c["rect"], c["flags"]


def shifted(c, di, dj):
    """case c moved by the lattice vector of di columns and dj rows (dj even, so that the odd rows stay odd)"""
    p, q, _ = c["lattice"]
    v = np.array([di * p, dj * q], np.int64)
    x0, y0, x1, y1 = c["rect"]
    return dict(c, ring_pts=(c["ring_pts"].astype(np.int64) + v).astype(np.int32), rect=(x0 + v[0], y0 + v[1], x1 + v[0], y1 + v[1])), v


# ------------------------------------------------------------------ the whole tool
# a square with a fill, an unfilled circle, and a rectangle of another colour painted over the square's corner
TOOL_SVG = b"""<svg xmlns="http://www.w3.org/2000/svg" width="200" height="200" viewBox="0 0 200 200">
 <rect x="10" y="10" width="100" height="100" fill="#88f" stroke="#00f"/>
 <circle cx="150" cy="150" r="30" fill="none" stroke="#000"/>
 <rect x="80" y="80" width="60" height="50" fill="#f88" stroke="#f00"/>
</svg>
"""
TOOL_SVG_DOTS_ONLY = b"""<svg xmlns="http://www.w3.org/2000/svg" width="200" height="200" viewBox="0 0 200 200">
 <rect x="10" y="10" width="100" height="100" fill="#88f" stroke="#00f"/>
</svg>
"""
TOOL_ARGS = ["--scale", "1", "--margin-mm", "0", "--steps-per-mm", "10"]


class StippleDouble:
    """stipple_fn of orip.svg.build_stream_from_svg through the doubles: the rings converted by occlude_double.rings_to_steps, the pass by stipple_double"""
    def __init__(self): self.calls = 0; self.out = None; self.args = None

    def __call__(self, paths, ring_sub, ring_group, m, clamp, lattice, inset, rect, flags):
        import occlude_double as OD
        r_off, r_pts = OD.rings_to_steps(np.asarray(paths[0]), np.asarray(paths[1]), np.asarray(ring_sub).tolist(), m, clamp)
        self.args = dict(ring_off=r_off, ring_pts=r_pts, ring_group=np.asarray(ring_group), clamp=clamp, lattice=lattice, inset=inset, rect=rect, flags=flags)
        self.out = SD.stipple(r_off, r_pts, ring_group, lattice, inset, rect, flags)
        self.calls += 1
        return self.out
