"""The inputs of tests/contour_cases.py have the properties they are built for -- proven on the oracle alone (O.thin_rot, O.trace, O.stage04) with
the numpy helpers of contour_cases (pixel degrees, maximal degree-2 chains), so that tests/test_gpu_contour_cases.py compares the device on maps
that do reach chain_jump's thresholds, every row loader of load_tile, the chain-list capacity and the thinning cap.  Chain lengths are measured
on the thinned skeleton, not on the drawing.  No case is dropped at run time: a generator that misses a property fails here."""
import numpy as np
import pytest

from oracle import oracle as O
import contour_cases as C

_cache = {}


def fam(name):
    """(names, stack, skeletons) of a family, computed once"""
    if name not in _cache:
        names, st = C.FAMILIES[name]()
        _cache[name] = (names, st, [O.thin_rot(e) for e in st])
    return _cache[name]


def _thin_iterations(e):
    """(iterations the oracle's thinning ran, skeleton): the count includes the last one, which deletes nothing unless the cap of 120 ended the loop"""
    a = np.ascontiguousarray(e, np.uint8); out = np.empty_like(a)
    return O.lib().orc_thin_rot(O._p(a), O._p(out), a.shape[0], a.shape[1]), out


def _ends(sk, length):
    """end pixels (y, x) of the listed chains of exactly `length` pixels"""
    return [p for pix, has_end in C.chains(sk) if has_end and len(pix) == length for p in (pix[0], pix[-1])]


# ---------------------------------------------------------------- every family
@pytest.mark.parametrize("name", list(C.FAMILIES))
def test_family_is_well_formed_and_every_map_keeps_a_path(name):
    names, st, _ = fam(name)
    assert st.dtype == np.uint8 and st.ndim == 3 and 1 <= st.shape[0] <= 16 and st.shape[0] == len(names) == len(set(names))
    assert st.shape[1] <= 324 and st.shape[2] <= 324
    for n, e in zip(names, st):
        assert len(O.stage04(e)) >= 1, (name, n, "thins to nothing that is kept")


@pytest.mark.parametrize("name", C.CLOSED + [f"place_{k}_{W}" for k in ("theta", "d64", "d129") for W in C.WIDTHS])
def test_closed_members_have_no_endpoint(name):
    names, _, sks = fam(name)
    for n, sk in zip(names, sks):
        assert int((C.degrees(sk) == 1).sum()) == 0, (name, n)


# ---------------------------------------------------------------- chain lengths
@pytest.mark.parametrize("transposed", [False, True])
def test_thetas_have_three_chains_of_every_length(transposed):
    found = {}
    for part in "ab":
        names, st, sks = fam(("thetaT_" if transposed else "theta_") + part)
        for n, sk in zip(names, sks):
            assert O.ccl8(sk)[0] - 1 == 1, (n, "one component")
            found[int(n.rsplit("_", 1)[1])] = sorted((len(p) for p, e in C.chains(sk) if e), reverse=True)[:3]
            steps = {abs((b[0] - a[0]) * st.shape[2] + b[1] - a[1]) for p, e in C.chains(sk) if len(p) >= 8 for a, b in zip(p[:-1], p[1:])}
            assert steps == ({st.shape[2]} if transposed else {1}), (n, steps)          # +-W when transposed, +-1 upright
    assert sorted(found) == sorted(C.CHAIN_LENGTHS)
    for n, top in found.items():
        assert top == [n, n, n], (n, top)
    print("theta chain lengths:", found)


def test_diamond_chain_lengths_straddle_24_and_64():
    names, st, sks = fam("diamonds")
    lengths = set()
    for (r, f), n, sk in zip(C.DIAMONDS, names, sks):
        got = sorted(len(p) for p, e in C.chains(sk) if e)
        assert got == [2 * r - 5 + f, 2 * r - 3 + f, 2 * r - 3 + f], (n, got)
        lengths.update(got)
        W = st.shape[2]
        steps = {abs((b[0] - a[0]) * W + b[1] - a[1]) for p, e in C.chains(sk) if len(p) == 2 * r - 3 + f for a, b in zip(p[:-1], p[1:])}
        assert {W - 1, W + 1} <= steps, (n, steps)                                      # the diagonals: +-(W +- 1)
    assert {21, 22, 23, 24, 25, 26} <= lengths and {61, 62, 63, 64, 65, 66} <= lengths and {77, 75, 129} <= lengths, sorted(lengths)
    print("diamond chain lengths:", sorted(lengths))


def test_chordless_diamond_is_a_ring_without_chain_end():
    names, _, sks = fam("diamonds")
    sk = sks[names.index("diamond_ring")]
    ch = C.chains(sk)
    assert len(ch) == 1 and not ch[0][1] and len(ch[0][0]) == 4 * C.RING_R == int((sk > 0).sum())
    assert C.listed_lengths(sk) == []


def test_diamond_walks_start_inside_a_chain():
    """the raster-first pixel (where the leftover walk of the component starts) is the apex: degree 2, with a chain pixel on either side"""
    for name in ["diamonds"] + [f"place_d129_{W}" for W in C.WIDTHS]:
        names, _, sks = fam(name)
        for n, sk in zip(names, sks):
            if "T_" in n or n == "diamond_ring":
                continue                                                    # transposed: the raster-first pixel is a side corner; the ring has no end at all
            y, x = (int(v) for v in np.argwhere(sk > 0)[0])
            assert C.degrees(sk)[y, x] == 2, (name, n)
            pix = [p for p, _ in C.chains(sk) if (y, x) in p][0]
            assert 0 < pix.index((y, x)) < len(pix) - 1, (name, n, "home is an end pixel")


def test_loops_have_listed_chains_with_corners():
    for name, members in (("loops", None), ("open", ("spiral_closed", "spiral_closed_rot"))):
        names, _, sks = fam(name)
        for n, sk in zip(names, sks):
            if (members and n not in members) or n.endswith("_sq"):
                continue
            turning = [p for p, e in C.chains(sk) if e and len(p) >= C.CHAIN_MIN and len({(b[0] - a[0], b[1] - a[1]) for a, b in zip(p[:-1], p[1:])}) >= 2]
            assert turning, (name, n)
    names, _, sks = fam("open")
    for n in ("spiral_closed", "spiral_closed_rot"):
        assert max(C.listed_lengths(sks[names.index(n)])) >= 500, n              # multi-hundred-pixel chains for the leftover walk


# ---------------------------------------------------------------- placement
@pytest.mark.parametrize("W", C.WIDTHS)
def test_placement_puts_chain_ends_on_every_target(W):
    groups = {"theta": [f"place_theta_{W}"], "diamond": [f"place_d64_{W}", f"place_d129_{W}"]}
    for member, fams in groups.items():
        for length in (64, 129):
            xs, ys = set(), set()
            for f in fams:
                names, st, sks = fam(f)
                assert st.shape[1:] == (C.PLACE_H, W)
                for n, sk in zip(names, sks):
                    if "border" in n or "corner" in n or "centre" in n:
                        continue
                    for y, x in _ends(sk, length):
                        xs.add(x); ys.add(y)
            assert set(C.TARGETS) <= xs, (member, length, "x", sorted(set(C.TARGETS) - xs))
            assert set(C.TARGETS) <= ys, (member, length, "y", sorted(set(C.TARGETS) - ys))


@pytest.mark.parametrize("W", C.WIDTHS)
def test_placement_touches_every_border_and_keeps_its_distance(W):
    H = C.PLACE_H
    for f, layers, length in ((f"place_theta_{W}", ("theta_64_borders",), 64), (f"place_theta_{W}", ("theta_129_borders",), 129),
                              (f"place_d64_{W}", ("diamond64_corners_a", "diamond64_corners_b"), 64)):
        names, _, sks = fam(f)
        touched = np.zeros(4, bool)
        for n in layers:
            sk = sks[names.index(n)] > 0
            touched |= np.array([sk[0].any(), sk[H - 1].any(), sk[:, 0].any(), sk[:, W - 1].any()])
            assert length in C.listed_lengths(sk), (f, n)
        assert touched.all(), (f, layers, touched)
    for W129 in (f"place_d129_{W}",):                                          # the 129 diamonds touch rows 0 and H-1 and columns 0 and W-1 among their target layers
        names, _, sks = fam(W129)
        anysk = np.any([s > 0 for s in sks], axis=0)
        assert anysk[0].any() and anysk[H - 1].any() and anysk[:, 0].any() and anysk[:, W - 1].any()
    names, _, sks = fam(f"place_d64_{W}")
    ys, xs = np.nonzero(sks[names.index("diamond64_centre")])
    assert min(ys.min(), xs.min(), H - 1 - ys.max(), W - 1 - xs.max()) > 64
    names, _, sks = fam(f"place_theta_{W}")
    ys, xs = np.nonzero(sks[0])
    assert min(ys.min(), xs.min()) < 24


def test_every_row_loader_has_its_width_and_a_window_inside_the_image():
    """load_tile: 16-byte loads need W % 16 == 0, 4-byte loads W % 4 == 0, and both a window inside the image: tx0 = ((x - 24 + lead) >> 4) << 4 with
    |lead| <= 16 lies in [0, W - 64] for every cursor column x in [40, W - 56].  A cursor nearer than 24 px to the left border has tx0 < 0: bytes."""
    assert [w for w in C.WIDTHS if w % 16 == 0] and [w for w in C.WIDTHS if w % 4 == 0 and w % 16] and len([w for w in C.WIDTHS if w % 2]) >= 2
    for W in C.WIDTHS:
        for f in (f"place_theta_{W}", f"place_d64_{W}", f"place_d129_{W}"):
            _, _, sks = fam(f)
            xs = np.array([x for sk in sks for p, e in C.chains(sk) if e and len(p) >= C.CHAIN_MIN for _, x in p])
            assert ((xs >= 40) & (xs <= W - 56)).any() and (xs < 24).any(), (f,)


# ---------------------------------------------------------------- open paths, small things, narrow images
def test_open_paths_are_what_they_say():
    names, st, sks = fam("open")
    for n in ("spiral", "spiral_T", "serpentine", "serpentine_T"):
        sk = sks[names.index(n)]; deg = C.degrees(sk)
        assert (deg == 1).sum() == 2 and (deg > 2).sum() == 0 and O.ccl8(sk)[0] - 1 == 1, n            # one open path
        assert (sk > 0).sum() >= 3000, n
    for n in ("spiral_closed", "spiral_closed_rot"):
        deg = C.degrees(sks[names.index(n)])
        assert (deg > 2).sum() > 0 and (deg == 1).sum() >= 1, n
    W = st.shape[2]
    for n, want_steps in (("lines", {1, W, W + 1}), ("lines_anti", {W - 1})):
        sk = sks[names.index(n)]
        lens = sorted(len(p) + 2 for p, e in C.chains(sk) if e)                                       # a line of n px: n - 2 degree-2 pixels between its endpoints
        assert lens == sorted(list(C.LINE_LENGTHS) * len(want_steps)), (n, lens)
        steps = {abs((b[0] - a[0]) * W + b[1] - a[1]) for p, e in C.chains(sk) for a, b in zip(p[:-1], p[1:])}
        assert steps == want_steps, (n, steps)
    for n in ("zigzag", "zigzag_T"):
        sk = sks[names.index(n)]
        steps = {abs((b[0] - a[0]) * W + b[1] - a[1]) for p, e in C.chains(sk) for a, b in zip(p[:-1], p[1:])}
        assert steps == {W - 1, W + 1}, (n, steps)                                                   # both diagonals, walked from either end


def test_small_things():
    names, _, sks = fam("small_things")
    sk = sks[names.index("comb")]
    assert (C.degrees(sk) == 1).sum() >= 60 and [l for l in C.listed_lengths(sk) if 26 <= l <= 40]   # many teeth, a few long ones that are listed
    for n in ("ladder", "ladder_T"):
        sk = sks[names.index(n)]
        assert (C.degrees(sk) == 1).sum() == 0 and C.listed_lengths(sk) == [], n
    sk = sks[names.index("specks")]
    assert O.ccl8(sk)[0] - 1 >= 900                                                                  # NC large, nearly every path below the 5-point filter


@pytest.mark.parametrize("W", [1, 2, 3])
def test_narrow_images(W):
    names, st, sks = fam(f"narrow{W}")
    assert st.shape[2] == W and st.shape[1] == C.NARROW_H
    if W >= 2:
        # a listed chain whose two ends border junction pixels only: no endpoint walk enters it (an endpoint walk stops on the first junction pixel it
        # steps on), so a LEFTOVER walk reaches a listed chain in a two-column image: chain_jump's direction decode must hold for W = 2
        for n in ("zigzag_junctions", "column_junctions"):
            sk = sks[names.index(n)]; deg = C.degrees(sk); fg = sk > 0
            ok = []
            for pix, has_end in C.chains(sk):
                if not has_end or len(pix) < C.CHAIN_MIN:
                    continue
                outside = [(y + dy, x + dx) for y, x in (pix[0], pix[-1]) for dy, dx in C._N8
                           if 0 <= y + dy < sk.shape[0] and 0 <= x + dx < W and fg[y + dy, x + dx] and deg[y + dy, x + dx] != 2]
                ok.append(all(deg[q] >= 3 for q in outside))
            assert any(ok), (W, n)
        sk = sks[names.index("zigzag_junctions")]
        steps = {(b[0] - a[0]) * W + b[1] - a[1] for p, e in C.chains(sk) if e and len(p) >= C.CHAIN_MIN for a, b in zip(p[:-1], p[1:])}
        if W == 2:
            assert {1, 3} <= {abs(s) for s in steps}, steps                                         # +W - 1 = +1: a step down-left that looks like a step right
    if W == 3:
        sk = sks[names.index("ladder30")]
        assert (C.degrees(sk) == 1).sum() == 0 and len(C.listed_lengths(sk)) >= 6


# ---------------------------------------------------------------- thinning
def test_small_squares_end_on_both_parities():
    names, st, _ = fam("small_squares")
    deleting = []
    for n, e in zip(names, st):
        it, sk = _thin_iterations(e)
        assert np.array_equal(O.thin_rot(sk), sk), n                         # ended because nothing was deleted
        deleting.append(it - 1)
    print("deleting iterations of the small squares:", dict(zip(C.SMALL_SQUARES, deleting)))
    assert min(deleting) == 1 and max(deleting) == 6 and {d % 2 for d in deleting} == {0, 1} and deleting == sorted(deleting), deleting


def test_square_300_runs_into_the_cap():
    names, st, sks = fam("thick")
    it, sk = _thin_iterations(st[names.index("square_300")])
    assert it == C.THIN_CAP
    assert not np.array_equal(O.thin_rot(sk), sk)                            # one more round of iterations would still delete: the cap decides the result
    assert (sk > 0).sum() > 3000
    it, sk = _thin_iterations(st[names.index("disc_60")])
    assert 30 < it < C.THIN_CAP and np.array_equal(O.thin_rot(sk), sk)


# ---------------------------------------------------------------- capacity
def test_capacity_pair_exceeds_both_limits_twice():
    _, small = C.capacity_small()
    M = int(sum((O.thin_rot(e) > 0).sum() for e in small))
    assert 1 <= M <= 16
    assert len(O.stage04(small[0])) >= 1
    names, crowded = C.capacity_crowded()
    assert crowded.shape == (8, 256, 256)
    n_ends = n_cpix = 0
    for e in crowded:
        sk = O.thin_rot(e)
        for pix, has_end in C.chains(sk):
            if has_end:
                n_ends += len({pix[0], pix[-1]})                              # one list entry per end pixel (a chain of one pixel has one)
                if len(pix) >= C.CHAIN_MIN:
                    n_cpix += len(pix) + 2                                    # a sentinel on either side
    print(f"small M = {M}: room for {C.cap_ends_after(M)} ends, {C.cap_cpix_after(M)} chain pixels; crowded has {n_ends} ends, {n_cpix} chain pixels")
    assert n_ends > 2 * C.cap_ends_after(M), (n_ends, C.cap_ends_after(M))
    assert n_cpix > 2 * C.cap_cpix_after(M), (n_cpix, C.cap_cpix_after(M))
