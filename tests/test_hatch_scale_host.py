"""The cases of tests/hatch_scale_cases.py without a GPU: with the counting functions of that file and the doubles alone, every case reaches what it is named
after -- its units (blocks of 64 samples, chunks of 64 slots, pairs in reach) and the passes of the capped grid over them, the block at which the second
family begins, the batch of 64 in which a hiding shape is met, the rounds of pointer jumping and the length of the chain they run over -- and the mirrored
launch constants are those of the three sources.  fill_double.fill_mask_numpy is pinned here to the sequential fill_double.fill_mask, by equality, on every
case of tests/fill_cases.py.  tests/test_gpu_hatch_scale.py then runs the same cases on the device."""
import os
import re

import numpy as np
import pytest

import fill_cases as FC
import fill_double as FD
import hatch_link_cases as LC
import hatch_link_double as LD
import hatch_scale_cases as HS
import stipple_cases as SC
import stipple_double as SD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_FILL = FC.cases()
_MEMO = {}


def _src(name):
    return open(os.path.join(ROOT, "omnirevolve-image-processor_amd", "csrc", name)).read()


def _stipple(name, c=None):
    """the double's answer for a named case, computed once"""
    if name not in _MEMO:
        _MEMO[name] = SD.stipple(*SC.args(HS.stipple_cases()[name] if c is None else c))
    return _MEMO[name]


def _undirected(seg):
    """the segments as a sorted list, each from its lower end"""
    return sorted(min((a, b, c, d), (c, d, a, b)) for a, b, c, d in seg.tolist())


def _link(name):
    if name not in _MEMO:
        _MEMO[name] = LD.hatch_link(*LC.args(HS.link_cases()[name]))
    return _MEMO[name]


def test_constants_are_the_kernels():
    fl, st, hl = _src("fill.hip"), _src("gcode_stipple.hip"), _src("gcode_link.hip")
    assert int(re.search(r"constexpr int FL_BLOCKS = (\d+);", fl).group(1)) == HS.FL_BLOCKS
    assert int(re.search(r"constexpr int ST_BLOCKS = (\d+);", st).group(1)) == HS.ST_BLOCKS
    assert int(re.search(r"constexpr int HL_BLOCKS = (\d+);", hl).group(1)) == HS.HL_BLOCKS
    # the fill: blocks of 256 threads, FL_WAVES waves each, a wave per block of samples, over min(cdiv(Z, FL_WAVES), FL_BLOCKS) blocks; both strided kernels
    assert "const dim3 b(256), gw((unsigned)std::min<u64>((g.Z + 3) / 4, FL_BLOCKS));" in fl and HS.FL_WAVES == 256 // 64 == 4
    assert fl.count("for (u64 z = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); z < g.Z; z += (u64)gridDim.x * 4)") == 2
    assert "hipLaunchKernelGGL(k_fl_sample, gw, b," in fl and "hipLaunchKernelGGL(k_fl_scatter, gw, b," in fl
    # the stipple: blocks of one wave over min(C, ST_BLOCKS) blocks; both strided kernels; the shapes above 64 at a time
    assert "const dim3 gw((unsigned)std::min<u64>(C, ST_BLOCKS));" in st
    assert st.count("for (u64 ch = blockIdx.x; ch < C; ch += gridDim.x)") == 2
    assert "hipLaunchKernelGGL(k_st_test, gw, dim3(64)," in st and "hipLaunchKernelGGL(k_st_emit, gw, dim3(64)," in st
    assert "for (int64_t sb = g + 1; sb < sh.ns; sb += 64)" in st and HS.BATCH == 64
    # the hatch link: blocks of one wave over min(P, HL_BLOCKS) blocks; the rounds of pointer jumping
    assert "hipLaunchKernelGGL(k_hl_elig, dim3((unsigned)std::min<u64>(P, HL_BLOCKS)), dim3(64)," in hl
    assert "for (u64 q = blockIdx.x; q < P; q += gridDim.x)" in hl
    assert "int rounds = 0; while (((int64_t)1 << rounds) < nl) rounds++;" in hl


def test_passes_at_the_caps():
    assert [HS.passes(u, HS.ST_BLOCKS) for u in (0, 1, 8192, 8193, 16384, 16385)] == [0, 1, 1, 2, 2, 3]
    assert [HS.passes(u, HS.HL_BLOCKS) for u in (16384, 16385)] == [1, 2]
    assert [HS.passes(u, HS.FL_BLOCKS, HS.FL_WAVES) for u in (1, 5, 65536, 65537, 131072, 131073)] == [1, 1, 1, 2, 2, 3]
    # what the suite reached before: the largest cases of the three existing files stay in the first pass
    assert max(HS.fill_units(c) for c in SMALL_FILL.values()) < 1024
    assert max(HS.stipple_units(c) for c in SC.cases().values()) < 1024 < HS.ST_BLOCKS
    assert HS.link_units(LC.cases()["sixteen_shapes"]) < HS.HL_BLOCKS


# ================================================================================================ fill
@pytest.mark.parametrize("name", sorted(SMALL_FILL))
def test_fill_mask_numpy_is_fill_mask(name):
    a = FC.args(SMALL_FILL[name])
    seg, st = FD.fill_mask(*a)
    for kw in ({}, {"lines_at_once": 3}):                                                # whole and in slices of three lines
        got, gst = FD.fill_mask_numpy(*a, **kw)
        assert got.dtype == np.int32 and got.shape == seg.shape and np.array_equal(got, seg) and gst == st


def test_fill_mask_numpy_is_fill_mask_on_a_slice_of_the_large_cases():
    """the first 40 rows of the large canvases, where the sequential double is affordable: the same masks, placements and directions"""
    for name, c in HS.fill_cases().items():
        a = FC.args(dict(c, H=40))
        seg, st = FD.fill_mask(*a)
        got, gst = FD.fill_mask_numpy(*a)
        assert np.array_equal(got, seg) and gst == st and st["segments"] > 0, name


@pytest.mark.parametrize("name", sorted(HS.FILL_UNITS))
def test_fill_case_reaches_what_it_is_named_after(name):
    c = HS.fill_cases()[name]
    blocks, npass = HS.FILL_UNITS[name]
    assert HS.fill_units(c) == blocks and HS.passes(blocks, HS.FL_BLOCKS, HS.FL_WAVES) == npass
    assert blocks < 1 << 26                                                              # FL_MAX_BLOCKS: the call is not refused


def test_fill_cases_sit_on_the_cap():
    one_pass = HS.FL_BLOCKS * HS.FL_WAVES
    F = {n: HS.fill_families(c) for n, c in HS.fill_cases().items()}
    assert one_pass == 65536 and HS.FILL_UNITS["rows_cap"][0] == one_pass and HS.FILL_UNITS["rows_cap_plus_1"][0] == one_pass + 1
    for name, H in (("rows_cap", 131070), ("rows_cap_plus_1", 131072)):
        assert [(f["NW"], f["kmin"], f["L"]) for f in F[name]] == [(1, 0, H // 2 + 1)]
    assert [(f["NW"], f["kmin"], f["L"]) for f in F["rows_two_passes"]] == [(3, 0, 32769)]
    for name in ("rows_and_columns", "rows_and_columns_serpentine"):
        assert [(f["u"], f["NW"], f["kmin"], f["L"], f["first"]) for f in F[name]] == [((4096, 0), 3, 0, 32769, 0), ((0, 4096), 1024, -65, 66, 98307)]
    assert one_pass < 98307 < 2 * one_pass and 98307 % one_pass == 32771                 # the second family begins in the middle of the second pass
    assert [(f["NW"], f["kmin"], f["L"]) for f in F["oblique_tall"]] == [(4, -64, 17384)]
    assert [(f["NW"], f["kmin"], f["L"]) for f in F["oblique_tall_negative_u"]] == [(4, -17383, 17384)]      # x-major with d < 0: every k that counts is negative
    for name in ("oblique_tall", "oblique_tall_negative_u"):
        num, den, dx, dy = HS.fill_cases()[name]["place"]
        assert den > 1 and dx < 0 and dy < 0


@pytest.mark.parametrize("name", sorted(HS.FILL_UNITS))
def test_fill_case_answers(name):
    """the numpy double on the large case: the scans behind the kernels are longer than 65 536 words, runs cross the block boundaries and end at the canvas
    edges, some are short; where the closed form applies it is a second, independent answer"""
    c = HS.fill_cases()[name]
    seg, st = FD.fill_mask_numpy(*FC.args(c))
    assert st["runs"] == st["short"] + st["segments"] == st["short"] + len(seg) and st["segments"] > 30000
    assert HS.fill_units(c) + 1 > 65536                                                  # the scan over the blocks
    fams = HS.fill_families(c)
    assert 0 <= sum(f["L"] for f in fams) - st["lines"] <= len(fams)                     # the range the host lays out holds at most one line without a sample
    major = (seg[seg[:, 1] == seg[:, 3]] if name.startswith("rows") else seg)[:, [0, 2]]  # a of the lines along x
    lo, hi = major.min(1), major.max(1)
    assert ((lo <= 63) & (hi >= 64)).any() or c["W"] == 64
    if c["W"] > 128:
        assert ((lo <= 127) & (hi >= 128)).any()
    if name.startswith("oblique") or name.startswith("rows_cap"):
        assert st["short"] > 1000 and st["runs"] > 65536                                 # the scan over the runs as well
    if name in HS.CLOSED_FORM:
        want, runs, short = FC.rows_closed_form(c)
        assert np.array_equal(seg, want) and (st["runs"], st["short"]) == (runs, short)
    if name.endswith("serpentine"):
        plain = FD.fill_mask_numpy(*FC.args(HS.fill_cases()["rows_and_columns"]))
        assert plain[1] == st and not np.array_equal(plain[0], seg) and _undirected(plain[0]) == _undirected(seg)


# ================================================================================================ stipple
@pytest.mark.parametrize("name", sorted(HS.STIPPLE_UNITS))
def test_stipple_case_reaches_what_it_is_named_after(name):
    c = HS.stipple_cases()[name]
    chunks, npass = HS.STIPPLE_UNITS[name]
    assert HS.stipple_units(c) == chunks and HS.passes(chunks, HS.ST_BLOCKS) == npass
    st = _stipple(name)[2]
    shapes = HS.stipple_shapes(c)
    assert st["groups"] == len(shapes) and st["rows"] == sum(s["nrows"] for s in shapes) and st["dots"] == len(_stipple(name)[0]) > 0


def test_stipple_cases_sit_on_the_cap():
    C = HS.stipple_cases()
    one = HS.stipple_shapes(C["one_shape_two_passes"])
    assert [(s["nrows"], s["cols"], s["slots"], s["chunks"]) for s in one] == [(521, 1051, 547571, 8556)]
    st = _stipple("one_shape_two_passes")[2]
    assert (st["candidates"], st["near"], st["dots"]) == (544691, 5228, 539463)
    # an odd row's first and last place are read from the chunks of its two ends: rows are 1 051 slots, so one of them lies in another chunk than the dot's own,
    # and the rows around slot 64 * 8 192 lie in chunks of both passes
    assert C["one_shape_two_passes"]["lattice"][2] & 1 and C["one_shape_two_passes"]["flags"] & SD.SERPENTINE and 1051 > 64 and 547571 > 64 * HS.ST_BLOCKS
    sq = HS.stipple_shapes(C["squares_12000"])
    assert len(sq) == 12000 and max(s["chunks"] for s in sq) == 1 and sum(s["chunks"] == 0 for s in sq) == 1113      # every stride step lands in another shape
    assert not C["squares_12000"]["flags"] & SD.OCCLUDE
    for name, n in (("chunks_cap", HS.ST_BLOCKS), ("chunks_cap_plus_1", HS.ST_BLOCKS + 1)):
        assert [s["chunks"] for s in HS.stipple_shapes(C[name])] == [1] * n


@pytest.mark.parametrize("k", sorted(HS.COVER_AT))
def test_hidden_by_batch(k):
    name = f"hidden_by_batch_{k}"
    c = HS.stipple_cases()[name]
    cover = HS.COVER_AT[k]
    assert c["flags"] & SD.OCCLUDE and HS.batch_of(c, 0, cover) == k - 1 and len(HS.stipple_shapes(c)) == 140
    assert HS.batch_of(c, 0, cover - 1) == max(0, k - 2) and (k != 1 or HS.batch_of(c, 0, cover + 1) == 1)      # 64 is the last of its batch, 65 and 129 the first of theirs
    xy, grp, st = _stipple(name)
    assert st["hidden"] == 144 and st["dots"] > 0
    xy0 = {tuple(p) for p in xy[grp == 0].tolist()}
    bare = SD.stipple(*SC.args(HS.without(c, cover)))                                    # every hidden dot is hidden by that one shape alone
    assert bare[2]["hidden"] == 0 and bare[2]["dots"] - int((bare[1] == 0).sum()) == st["dots"] - len(xy0) - int((grp == cover).sum())
    bare0 = {tuple(p) for p in bare[0][bare[1] == 0].tolist()}
    assert xy0 < bare0 and len(bare0 - xy0) == 144 and all(400 < x < 900 and 300 < y < 800 for x, y in bare0 - xy0)
    box0 = HS.stipple_shapes(c)[0]["box"]                                                # the decoys never meet a chunk's box
    for s in HS.stipple_shapes(c)[1:]:
        b = s["box"]
        assert s["group"] == cover or b[1] > box0[3]


def test_hidden_by_the_second_batch_only():
    name = "hidden_by_the_second_batch_only"
    c = HS.stipple_cases()[name]
    assert [HS.batch_of(c, 0, g) for g in range(65, 70)] == [1] * 5 and len(HS.stipple_shapes(c)) == 70
    st = _stipple(name)[2]
    assert (st["groups"], st["candidates"], st["near"], st["hidden"], st["dots"]) == (70, 1248, 368, 230, 650)
    rest = c
    for g in range(65, 70):
        rest = HS.without(rest, g)
    assert SD.stipple(*SC.args(rest))[2]["hidden"] == 0                                  # nothing of the first batch hides anything


def test_first_batch_hides_all():
    """shape 1, of the first batch, hides every live dot of some chunks of shape 0; shape 70, of the second batch, meets the box of the same chunks: the loop
    over the batches has to stop for them, and go on for the chunks further down"""
    name = "first_batch_hides_all"
    c = HS.stipple_cases()[name]
    assert HS.batch_of(c, 0, 1) == 0 and HS.batch_of(c, 0, 70) == 1 and HS.batch_of(c, 1, 70) == 1
    xy, grp, st = _stipple(name)
    assert not (grp == 0).any() and st["hidden"] == 637                                  # both together hide all of shape 0
    only_a = SD.stipple(*SC.args(HS.without(c, 70)))
    live = {tuple(p) for p in SD.stipple(*SC.args(HS.without(HS.without(c, 70), 1)))[0].tolist()}      # the dots of shape 0 with nothing above it
    left = {tuple(p) for p in only_a[0][only_a[1] == 0].tolist()}
    s0 = HS.stipple_shapes(c)[0]
    x, y, ok = HS.slot_points(c, s0)
    ax0, ay0, ax1, ay1 = (HS.HALF_A[0][0], HS.HALF_A[0][1], HS.HALF_A[2][0], HS.HALF_A[2][1])
    bx0, by0, bx1, by1 = (HS.HALF_B[0][0], HS.HALF_B[0][1], HS.HALF_B[2][0], HS.HALF_B[2][1])
    stopped, went_on = 0, 0
    for ch in range(s0["chunks"]):
        pts = [(int(px), int(py)) for px, py, v in zip(x[64 * ch:64 * ch + 64], y[64 * ch:64 * ch + 64], ok[64 * ch:64 * ch + 64]) if v and (int(px), int(py)) in live]
        if not pts:
            continue
        meets_b = min(p[0] for p in pts) <= bx1 and max(p[0] for p in pts) >= bx0 and min(p[1] for p in pts) <= by1 and max(p[1] for p in pts) >= by0
        if all(ax0 < px < ax1 and ay0 < py < ay1 for px, py in pts):
            assert not any(p in left for p in pts)
            stopped += meets_b
        else:
            went_on += 1
    assert stopped >= 2 and went_on >= 4 and s0["chunks"] == 11


# ================================================================================================ hatch link
@pytest.mark.parametrize("name", sorted(HS.LINK_UNITS))
def test_link_case_reaches_what_it_is_named_after(name):
    c = HS.link_cases()[name]
    nl, pairs, npass, rounds = HS.LINK_UNITS[name]
    st = _link(name)[4]
    assert HS.link_units(c) == pairs == st["in_reach"] and st["lines"] == nl == len(c["off"]) - 1
    assert HS.passes(pairs, HS.HL_BLOCKS) == npass and HS.jump_rounds(nl) == rounds


def test_link_cases_sit_on_the_cap():
    assert [HS.LINK_UNITS[f"dense_{n}"][1] for n in (181, 182, 200)] == [n * (n - 1) // 2 for n in (181, 182, 200)] == [16290, 16471, 19900]
    assert 16290 < HS.HL_BLOCKS < 16471
    for n in (181, 182, 200):                                                            # a good share of the pairs is ineligible, and minima tie
        c, st = HS.link_cases()[f"dense_{n}"], _link(f"dense_{n}")[4]
        assert 0.3 * st["in_reach"] < st["eligible"] < 0.7 * st["in_reach"] and st["links"] > 30 and st["coincident"] > 5
    c = HS.link_cases()["dense_200"]
    S, E, _ = HS.link_lines(c)
    edges = LD.shape_edges(c["ring_off"].tolist(), [tuple(q) for q in c["ring_pts"].tolist()], c["ring_group"].tolist())[0]
    tied = 0
    for a in range(200):
        e = tuple(E[a].tolist())
        if not LD.inside(e, edges):
            continue
        d2 = sorted(int(((S[b] - E[a]) ** 2).sum()) for b in range(a + 1, 200) if not any(LD.segments_meet(e, tuple(S[b].tolist()), p, q) for p, q in edges))
        tied += len(d2) > 1 and d2[0] == d2[1]
    assert tied >= 10                                                                    # ENDs whose two best partners are equally far: the lower index decides


def test_link_chains():
    off, pts, moff, member, st = _link("tall_rectangle")
    assert (st["eligible"], st["links"], st["paths_out"]) == (22455, 2499, 1) and np.diff(moff).tolist() == [2500]
    assert 1 << 11 < 2500 <= 1 << 12                                                     # the chain needs the twelfth round
    off, pts, moff, member, st = _link("tall_u")
    assert (st["eligible"], st["links"], st["paths_out"]) == (22366, 2493, 2) and sorted(np.diff(moff).tolist()) == [1245, 1250]
    LC.check_consequences(HS.link_cases()["tall_u"], _link("tall_u"))
    assert max(int(np.diff(LD.hatch_link(*LC.args(c))[2]).max()) for n, c in LC.cases().items() if n in ("sixteen_shapes", "square")) < 64      # before: a few rounds


def test_the_largest_and_the_small_cases_exist():
    assert HS.LARGEST["fill"] in HS.fill_cases() and HS.LARGEST["stipple"] in HS.stipple_cases() and HS.LARGEST["link"] in HS.link_cases()
    assert HS.SMALL["fill"] in SMALL_FILL and HS.SMALL["stipple"] in SC.cases() and HS.SMALL["link"] in LC.cases()
    assert HS.FILL_UNITS[HS.LARGEST["fill"]][0] == max(v[0] for v in HS.FILL_UNITS.values())
    assert HS.LINK_UNITS[HS.LARGEST["link"]][1] == max(v[1] for v in HS.LINK_UNITS.values())
    slots = {n: sum(s["slots"] for s in HS.stipple_shapes(c)) for n, c in HS.stipple_cases().items()}
    assert slots[HS.LARGEST["stipple"]] == max(slots.values())
