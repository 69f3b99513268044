"""The stage 08-B cases of tests/skel_path_cases.py are what their names say.  Shown on the oracle alone, by walking the pieces of _post_skeleton_merge
(groups, ROI, stamp, thinning, labels, anchors, best path) one by one with the oracle's own primitives and restating the branch conditions of
csrc/vector08b.hip on them; the composition is held against O.post_skeleton_merge on every case.  CPU only."""
import numpy as np
import pytest

from oracle import oracle as O
import skel_path_cases as C
from util import same_polys

_FIELDS08 = ["tap_diam", "tap_max_dim", "min_keep", "tap_max_per", "tap_max_v", "sample_step", "tail_len_px", "col_rad", "grid_stride", "max_jump",
             "post_on", "post_brush", "post_step", "post_eps", "post_minlen", "W", "H", "brush_forbid"]
_BASE = dict(zip(_FIELDS08, O.derived08(dict(O.DEFAULTS, **C.CFG))))
CASES = C.cases()
BY_ID = {c[0]: c for c in CASES}


def prm_of(W, H, over):
    d = dict(_BASE); d.update(W=W, H=H); d.update(over)
    return d, np.array([d[k] for k in _FIELDS08], np.float64)


_memo = {}


def run(W, H, polys, over):
    """(stage-08 lines, taps, lines handed to 08-B, 08-B's merged lines before the travel reorder) under the overrides.  08-A draws the longest line
    first (stable) and moves single samples by a pixel, so the lines 08-B sees are the input's in order of length, nearly point for point."""
    key = (W, H, id(polys), tuple(sorted(over.items())))
    if key not in _memo:
        d, prm = prm_of(W, H, over)
        lines, taps = O.stage08_layer(polys, prm)
        kept, t0 = O.split_small_taps08(polys, prm)
        per = np.array([O.poly_perimeter(p) for p in kept], np.float32)
        forbid = np.zeros((H, W), np.uint8); cleaned = []
        for i in np.argsort(-per, kind="stable"):
            for seg in O.virtual_draw08(kept[i], forbid, prm):
                parts = O.split_jumps(seg, float(d["max_jump"]), 8)
                cleaned += parts if parts else [seg]
        lines2, t1 = O.split_small_taps08(cleaned, prm)
        merged = O.post_skeleton_merge(lines2, prm) if lines2 else []
        assert same_polys(O.reorder(merged, 0), lines) and t0 + t1 == taps, "the composition is the oracle's stage 08"
        _memo[key] = (lines, taps, lines2, merged, polys)
    return _memo[key][:4]


def analyse(lines2, d):
    """_post_skeleton_merge (08:376-469) piece by piece: per group its ROI, iteration count, skeleton, anchors and components in label order; per component
    its pixel count S, whether it holds each anchor, the anchored path, the chosen path and the resampled point count m"""
    b = int(d["post_brush"]); exp = 2 * b + 6; rad = max(1, b) // 2
    pts = [np.asarray(p).reshape(-1, 2) for p in lines2]
    boxes = [(q[:, 0].min() - exp, q[:, 1].min() - exp, q[:, 0].max() + exp, q[:, 1].max() + exp) for q in pts]
    per = np.array([O.poly_perimeter(p) for p in lines2], np.float32)
    groups = []
    for idxs in O.cluster_by_overlap(boxes):
        longest = idxs[0]
        for j in idxs:
            if per[j] > per[longest]:
                longest = j
        x0 = min(boxes[j][0] for j in idxs); y0 = min(boxes[j][1] for j in idxs); x1 = max(boxes[j][2] for j in idxs); y1 = max(boxes[j][3] for j in idxs)
        w, h = max(1, x1 - x0), max(1, y1 - y0)
        roi = np.zeros((h, w), np.uint8)
        for j in idxs:
            for a, c in zip(pts[j][:-1], pts[j][1:]):
                O.stamp_capsule(roi, a[0] - x0, a[1] - y0, c[0] - x0, c[1] - y0, rad)
        iters, sk = O.zs_std_count(roi, 48)
        g = dict(idxs=idxs, longest=longest, roi=(x0, y0, x1, y1), stamped=roi, iters=iters, sk=sk, comps=[], tie=int((per[idxs] == per[longest]).sum()))
        groups.append(g)
        ys, xs = np.nonzero(sk)
        if len(ys) == 0:
            continue
        anchors = []
        for ax, ay in (pts[longest][0], pts[longest][-1]):
            k = int(np.argmin((ys - (ay - y0)).astype(np.int64) ** 2 + (xs - (ax - x0)).astype(np.int64) ** 2))      # first in raster order on ties
            anchors.append((int(ys[k]), int(xs[k])))
        g["anchors"] = anchors
        num, lab = O.ccl8(sk)
        for cc in range(1, num):
            comp = (lab == cc)
            ha, hb = bool(comp[anchors[0]]), bool(comp[anchors[1]])
            anchored = O.bfs_path(comp, anchors[0], anchors[1]) if ha and hb else []
            path = O.component_best_path(comp, anchors[0] if ha else None, anchors[1] if hb else None, int(d["post_minlen"]))
            m = 0
            if len(path) >= 2:
                arr = np.array([(x0 + x, y0 + y) for y, x in path], np.float32)
                m = len(O.resample_arclen(arr, bool(len(path) > 2 and (arr[0] == arr[-1]).all()), float(d["post_step"]))[0])
            cy, cx = np.nonzero(comp)
            g["comps"].append(dict(S=int(comp.sum()), ha=ha, hb=hb, anchored=anchored, path=path, m=m, first=(int(cy[0]), int(cx[0])), mask=comp))
    return groups


_studies = {}


def study(name):
    """everything the tests below look at, computed once per case"""
    if name not in _studies:
        _, W, H, polys, over, caps = BY_ID[name]
        lines, taps, lines2, merged = run(W, H, polys, over)
        d, _ = prm_of(W, H, over)
        _studies[name] = dict(lines=lines, taps=taps, lines2=lines2, merged=merged, groups=analyse(lines2, d), d=d, caps=caps)
    return _studies[name]


def xy(p):
    return np.asarray(p).reshape(-1, 2)


# ---------------------------------------------------------------- the device's rules, restated
def caps_at(step, hook):
    """(cap0, cap1) of b_paths: the largest components of the small and the large LDS class at this step, under an ORIP_COMP_CAPS value"""
    ratio = 1.41422 / step; room = min(step, 65536.0)

    def cap_of(budget):
        a = (budget - 13.0 * (room + 4.0) - 64.0) / (25.0 + 13.0 * ratio); b = (budget - 13.0 * 4.0 - 64.0) / (25.0 + 13.0 * (ratio + 1.0))
        return int(min(max(0.0, a, b), 65000.0)) & ~7
    cap0, cap1 = cap_of(32 * 1024), cap_of(160 * 1024)
    if hook:
        a, b = (int(v) for v in hook.split(","))
        if 8 <= a <= b:
            cap0, cap1 = min(cap0, a & ~7), min(cap1, b & ~7)
    return cap0, cap1


def class_of(S, step, hook):
    cap0, cap1 = caps_at(step, hook)
    return 0 if S <= cap0 else 1 if S <= cap1 else 2


_OFFS = [(-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1)]      # 08:252


def chunked_sweep(comp, src):
    """bfs_wave's full sweep from src, eight queue nodes (64 (node, direction) pairs) at a time, the lowest pair winning a pixel that several reach (which is
    plain FIFO order): (pixels that several pairs of one chunk reached, those of them whose lowest and highest pair belong to different nodes, the last
    pixel dequeued)"""
    h, w = comp.shape
    seen = np.zeros((h, w), bool); seen[src] = True
    que = [src]; head = 0; dups = other_parent = 0
    while head < len(que):
        nodes = que[head:head + 8]; head += len(nodes)
        pairs = {}                                            # new pixel -> the slots of the pairs that reach it, in pair order
        for slot, (y, x) in enumerate(nodes):
            for dy, dx in _OFFS:
                v = (y + dy, x + dx)
                if 0 <= v[0] < h and 0 <= v[1] < w and comp[v] and not seen[v]:
                    pairs.setdefault(v, []).append(slot)
        for v, slots in pairs.items():                        # (dicts keep insertion order: the order of each pixel's lowest pair)
            seen[v] = True; que.append(v)
            dups += len(slots) > 1; other_parent += slots[0] != slots[-1]
    return dups, other_parent, que[-1]


def block_key(first_pixels, wb, oy=0, ox=0):
    return min(((y + oy) >> 1) * wb + ((x + ox) >> 1) for y, x in first_pixels)


def comp_keys(g, absolute=False):
    """k_comp_keys: per component the smallest 2 x 2 block index, counted from the ROI's corner (or, wrongly, from the canvas's)"""
    x0, y0, x1, y1 = g["roi"]; wb = (max(1, x1 - x0) + 1) >> 1
    out = []
    for c in g["comps"]:
        ys, xs = np.nonzero(c["mask"])
        out.append(block_key(zip(ys.tolist(), xs.tolist()), wb, y0 if absolute else 0, x0 if absolute else 0))
    return out


# ---------------------------------------------------------------- every case
def test_the_default_classes():
    assert caps_at(6.0, None) == (1160, 5824)
    assert caps_at(6.0, "8,8") == (8, 8) and caps_at(6.0, "133,141") == (128, 136) and caps_at(6.0, "7,9") == (1160, 5824)


_CLASS_NAMED = {"eps0-step1-oblique": 1, "step1.0-diag": 0, "step1.2-diag": 0}      # (764 px against 752 at step 1: the large LDS class at two points per pixel)
_CLASS_SUFFIX = {"small": 0, "large": 1, "global": 2, "600": 2, "cap0_eq": 0, "cap0_plus1": 1, "cap1_eq": 1, "cap1_plus1": 2}


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_case_is_what_it_says(name):
    _, W, H, polys, over, caps = BY_ID[name]
    q = np.concatenate([xy(p) for p in polys])
    assert q.min() >= 0 and q[:, 0].max() < W and q[:, 1].max() < H, "the geometry stays inside the canvas"
    assert set(over) <= {"post_brush", "post_step", "post_eps", "post_minlen"}
    s = study(name)
    assert len(s["lines2"]) >= 1, "stage 08-A hands lines to 08-B"
    assert sum(len(g["comps"]) for g in s["groups"]) >= 1, "there is a skeleton"
    if over:
        at_defaults = run(W, H, polys, {})
        same = same_polys(s["lines"], at_defaults[0]) and s["taps"] == at_defaults[1]
        assert same == (name in C.SAME_AS_DEFAULT), "an override changes the result, unless an identity is stated"
    else:
        assert len(s["lines"]) >= 1
    suffix = name.rsplit("-", 1)[-1]
    if suffix in _CLASS_SUFFIX:
        need = max(2, int(s["d"]["post_minlen"]))
        big = [c["S"] for g in s["groups"] for c in g["comps"] if c["S"] >= need]
        assert big and {class_of(S, float(s["d"]["post_step"]), caps) for S in big} == {_CLASS_SUFFIX[suffix]}, (big, caps_at(float(s["d"]["post_step"]), caps))
    elif name in _CLASS_NAMED:
        assert {class_of(c["S"], float(s["d"]["post_step"]), caps) for g in s["groups"] for c in g["comps"]} == {_CLASS_NAMED[name]}
    elif caps is None and not over:
        assert {class_of(c["S"], 6.0, None) for g in s["groups"] for c in g["comps"]} == {0}


def test_the_whole_companion_is_small():
    assert len(CASES) < 120 and max(max(c[1], c[2]) for c in CASES) <= 800


# ---------------------------------------------------------------- path choice
def test_tie_for_the_longest_line():
    a, b = study("tie_first"), study("tie_second")
    for s in (a, b):
        (g,) = s["groups"]
        assert g["tie"] == 2 and g["longest"] == g["idxs"][0], "two lines of one perimeter: the lower index is the longest"
        (c,) = g["comps"]
        assert c["ha"] and c["hb"] and c["path"] == c["anchored"] and len(c["path"]) == C.TIE_PATH, "the anchored path is taken"
    assert same_polys(a["lines2"], b["lines2"][::-1])
    pa, pb = xy(a["merged"][0]), xy(b["merged"][0])
    assert pa[0, 0] < pa[-1, 0] and pb[0, 0] > pb[-1, 0], "the merged line runs the way of the first of the two"
    assert (pa[0].tolist(), pa[-1].tolist(), pb[0].tolist(), pb[-1].tolist()) == ([23, 101], [112, 101], [114, 102], [25, 101])


def test_both_anchors_on_one_pixel():
    for name in ("hairpin", "lollipop"):
        (g,) = study(name)["groups"]
        (c,) = g["comps"]
        assert g["anchors"][0] == g["anchors"][1] and c["ha"] and len(c["anchored"]) == 1, name
        assert len(c["path"]) >= 32, "a one-pixel path is too short: the diameter"
    (c,) = study("lollipop")["groups"][0]["comps"]
    assert chunked_sweep(c["mask"], c["first"])[1] > 0, "the search meets itself on the ring"


def test_anchored_path_too_short_diameter_taken():
    for name, where in (("ring", None), ("out_and_back", 250), ("out_and_back_tail", 400)):
        s = study(name)
        (g,) = s["groups"]
        (c,) = g["comps"]
        assert c["ha"] and c["hb"] and g["anchors"][0] != g["anchors"][1]
        assert 2 <= len(c["anchored"]) < 32 <= len(c["path"]), (name, len(c["anchored"]), len(c["path"]))
        if where:
            assert abs(int(xy(s["merged"][0])[:, 0].max()) - where) < 8, "the diameter reaches the far end"
    assert len(xy(study("ring")["merged"][0])) == 13


def test_anchors_outside_the_component():
    s = study("anchors_outside")
    (g,) = s["groups"]
    assert len(g["idxs"]) == 2 and [(c["ha"], c["hb"]) for c in g["comps"]] == [(True, True), (False, False)]
    assert g["comps"][0]["path"] == g["comps"][0]["anchored"] and g["comps"][1]["anchored"] == [] and len(g["comps"][1]["path"]) >= 32
    assert len(s["merged"]) == 2


def _order_is_visible(s):
    """the two merged lines tie for the longest, and the travel reorder gives another list when they come the other way round"""
    a, b = s["merged"]
    assert np.float32(O.poly_perimeter(a)) == np.float32(O.poly_perimeter(b))
    assert same_polys(O.reorder(s["merged"], 0), s["lines"]) and not same_polys(O.reorder(s["merged"][::-1], 0), s["lines"])


def test_component_order_is_block_raster_from_the_roi_corner():
    for dy in (0, 1):
        for dx in (0, 1):
            s = study(f"order_dx{dx}_dy{dy}")
            (g,) = s["groups"]
            ka, kb = comp_keys(g)
            assert ka < kb and len(s["merged"]) == 2 and g["roi"][1] % 2 == 1
            assert xy(s["merged"][0])[:, 0].max() < 225 < xy(s["merged"][1])[:, 0].min(), "A, the left one, comes first"
            assert g["comps"][1]["first"][0] < g["comps"][0]["first"][0], "although B's first pixel lies higher"
            ja, jb = comp_keys(g, absolute=True)
            assert jb < ja, "a key from canvas coordinates puts B first"
            _order_is_visible(s)
    s = study("order_control")
    (g,) = s["groups"]
    assert comp_keys(g)[0] < comp_keys(g)[1] and g["comps"][0]["first"][1] > 180, "the first component in label order is B"
    assert xy(s["merged"][0])[:, 0].min() > 225 > xy(s["merged"][1])[:, 0].max(), "two rows lower, A comes second"
    _order_is_visible(s)


def test_a_group_inside_another_groups_roi():
    """(the travel reorder hides the order of the two groups from the device test; what it sees is that each group thins on its own)"""
    for name, first_is_L in (("nested_L_first", True), ("nested_pair_first", False)):
        s = study(name)
        assert len(s["groups"]) == 2 and len(s["merged"]) == 2
        gl, gp = s["groups"] if first_is_L else s["groups"][::-1]
        assert len(gl["idxs"]) >= 3 and len(gp["idxs"]) == 2 and (0 in gl["idxs"]) == first_is_L
        assert gl["roi"][0] <= gp["roi"][0] and gl["roi"][1] <= gp["roi"][1] and gp["roi"][2] <= gl["roi"][2] and gp["roi"][3] <= gl["roi"][3], "the pair's boxes lie inside the L's ROI"
        assert not gl["stamped"][gp["roi"][1] - gl["roi"][1]:gp["roi"][3] - gl["roi"][1], gp["roi"][0] - gl["roi"][0]:gp["roi"][2] - gl["roi"][0]].any(), "and the L's ROI does not see them"
        assert (xy(s["merged"][0])[:, 1].max() > 300) == first_is_L, "the group ranks decide the order (the pair's line stays near y = 200)"


@pytest.mark.parametrize("name", ["x_cross", "hash", "comb", "ring", "lollipop", "brush100-line", "brush128-line"])
def test_junction_rich_skeletons_for_the_fifo_order(name):
    comps = [c for g in study(name)["groups"] for c in g["comps"]]
    c = max(comps, key=lambda c: c["S"])
    sk = c["mask"].astype(np.int32)
    nb = sum(np.roll(np.roll(np.pad(sk, 1), dy, 0), dx, 1)[1:-1, 1:-1] for dy, dx in _OFFS)
    assert ((nb >= 3) & c["mask"]).sum() >= 2 or name in ("ring",), "junction pixels"
    dups, other_parent, far = chunked_sweep(c["mask"], c["first"])
    assert dups > 0 and other_parent > 0, "pixels reached by several pairs of one chunk, from different nodes"
    assert chunked_sweep(c["mask"], far)[1] > 0


# ---------------------------------------------------------------- size classes
def test_class_boundaries_sit_on_the_component_size():
    for name, S in (("band_S8-cap0_eq", C.S8), ("band_S9-cap0_plus1", C.S9), ("band_S8-cap1_eq", C.S8), ("band_S9-cap1_plus1", C.S9)):
        s = study(name)
        (c,) = s["groups"][0]["comps"]
        cap0, cap1 = caps_at(6.0, s["caps"])
        assert c["S"] == S and (S == cap0 or S == cap0 + 1 or S == cap1 or S == cap1 + 1), (name, c["S"], cap0, cap1)
    assert C.S8 % 8 == 0 and C.S9 % 8 == 1


# ---------------------------------------------------------------- post_brush
_BATCH = {"brush26-line": (13, 16), "brush40-line": (17, 24), "brush60-line": (25, 32), "brush100-line": (48, 48), "brush128-line": (48, 48),
          # three lines 6 px across: the band is 6 px thicker than one line's, measured 24 and 34 iterations
          "brush40-horizontal_x64_y64": (17, 24), "brush40-vertical_x64_y64": (17, 24), "brush60-horizontal_x64_y64": (33, 36), "brush60-vertical_x64_y64": (33, 36),
          "brush128-borders": (48, 48), "brush129-borders": (48, 48)}


@pytest.mark.parametrize("name", sorted(_BATCH))
def test_thinning_runs_into_the_batch_it_is_meant_for(name):
    s = study(name)
    (g,) = s["groups"]
    lo, hi = _BATCH[name]
    assert lo <= g["iters"] <= hi, g["iters"]
    assert len(s["merged"]) >= 1, "and a line comes out of it"
    if lo == 48:
        assert not np.array_equal(O.zs_std_count(g["stamped"], 49)[1], g["sk"]), "unfinished: one more iteration would still change it"
        assert max(c["S"] for c in g["comps"]) > 1000, "a fat component"
    else:
        assert np.array_equal(O.zs_std_count(g["stamped"], g["iters"] - 1)[1], g["sk"]), "the last iteration found nothing to delete"
        assert not np.array_equal(O.zs_std_count(g["stamped"], g["iters"] - 2)[1], g["sk"]), "the one before it did"


def test_the_brush_table():
    """(iterations, pixels of the largest component): of the line itself, and of what stage 08-A makes of it (three pixels shorter)"""
    def row(lines2, b):
        (g,) = analyse(lines2, prm_of(400, 208, C.brush_fields(b))[0])
        return g["iters"], max(c["S"] for c in g["comps"])
    assert {b: row(C.LINE300, b) for b in (16, 26, 40, 60, 100, 128)} == {16: (9, 299), 26: (14, 297), 40: (21, 293), 60: (31, 289), 100: (48, 1137), 128: (48, 8581)}
    got = {b: row(study(f"brush{b}-line")["lines2"], b) for b in (26, 40, 60, 100, 128)}
    assert got == {26: (14, 294), 40: (21, 290), 60: (31, 286), 100: (48, 1021), 128: (48, 8381)}


def test_small_brushes_and_the_pad():
    assert [max(1, b) // 2 for b in (1, 2, 3, 128, 129, 130)] == [0, 1, 1, 64, 64, 65], "stamp radii; the pad holds 64"
    assert len(study("brush1")["groups"][0]["comps"]) > 50, "radius 0: an oblique line thins to single pixels"
    for name in ("brush128-borders", "brush129-borders"):
        s = study(name)
        (g,) = s["groups"]
        ys, xs = np.nonzero(g["stamped"])
        assert xs.min() + g["roi"][0] == -64 or ys.min() + g["roi"][1] == -64, "the band ends on the padded raster's first column / row"
        assert xs.min() > 0 and ys.min() > 0, "and the reference's ROI does not clip it"


# ---------------------------------------------------------------- post_step
@pytest.mark.parametrize("name", ["step1.0-diag", "step1.2-diag", "step1.0-diag-600", "step1.2-diag-global", "eps0.05-step1-diag", "eps0-step1-oblique", "eps0-step1-oblique-global"])
def test_step_below_sqrt2_resamples_to_more_points_than_pixels(name):
    s = study(name)
    (c,) = s["groups"][0]["comps"]
    assert c["m"] > c["S"] + 5, "more resample points than the component has pixels (+ 5: the room one entry per pixel left)"
    assert c["m"] <= 2 * c["S"]
    assert len(s["merged"]) == 1, "and the oracle keeps the line"
    if "diag" in name:
        assert 610 <= c["S"] <= 752, "inside the small class at this step, where the capped ratio lost it"
        p = xy(s["merged"][0])
        assert abs(p[0] - p[-1]).min() > 700


def test_float32_resample_positions():
    """t0 + i * delta in float32 (08:58): exact at 2.5 and 1.5 over these paths, rounded at 1.2 (delta is float32(1.2) and the products round again)"""
    i = np.arange(900, dtype=np.float32)
    assert (i * np.float32(2.5)).astype(np.float64).tolist() == (np.arange(900) * 2.5).tolist()
    assert ((i * np.float32(1.2)).astype(np.float64) != np.arange(900) * 1.2).sum() > 800
    for name in ("step2.5-diag_small", "step1.5-ring", "step2.5-ring", "step1.5-diag_small", "step1.2-diag"):
        assert len(study(name)["merged"]) == 1


def test_pass_through_of_a_path_shorter_than_the_step():
    a, b = study("step50-short"), study("step4000-short")
    for s in (a, b):
        (c,) = s["groups"][0]["comps"]
        assert c["m"] == len(c["path"]) == 26, "every pixel of the path passes through"
        assert [xy(p).tolist() for p in s["merged"]] == [[[101, 100], [126, 100]]]
    for name in ("step4000-band", "step4000-band-large", "step4000-band-global", "step1e300-band"):
        (c,) = study(name)["groups"][0]["comps"]
        assert c["m"] == len(c["path"]) == 295 and c["S"] == 299


# ---------------------------------------------------------------- post_eps
def test_eps_extremes():
    for name in ("eps0.05-ring", "eps0-ring"):
        s = study(name)
        (c,) = s["groups"][0]["comps"]
        assert len(xy(s["merged"][0])) > 0.75 * c["m"], "nearly every resampled point is kept"
    s = study("eps0.05-step1-diag")
    assert len(xy(s["merged"][0])) == 2, "an exact 45-degree skeleton resamples onto one straight line: the staircases below carry the kept count near m"
    s = study("eps0.05-step1-ring-global")
    (c,) = s["groups"][0]["comps"]
    assert len(xy(s["merged"][0])) > c["m"] // 2
    for name in ("eps0-step1-oblique", "eps0-step1-oblique-global"):
        s = study(name)
        (c,) = s["groups"][0]["comps"]
        assert len(xy(s["merged"][0])) > c["S"] + 5, "a staircase at a fine step and no tolerance: more points stay than the component has pixels"
    s = study("eps1e9-ring_comb")
    assert len(s["merged"]) == 2 and all(len(xy(p)) == 2 for p in s["merged"])


def test_two_components_with_more_kept_points_than_pixels():
    """the per-component offsets at two points per pixel, at a component base other than 0: BOTH components keep more points than they have pixels, so
    whichever comes first in the pixel list would write into the other's region if the regions held one point per pixel"""
    for name in ("eps0-step1-stairs2-small", "eps0-step1-stairs2-large", "eps0-step1-stairs2-global"):
        s = study(name)
        (g,) = s["groups"]
        assert len(g["comps"]) == 2 and len(s["merged"]) == 2
        assert [c["S"] for c in g["comps"]] == [718, 718] and [c["m"] for c in g["comps"]] == [771, 771]
        assert [len(xy(p)) for p in s["merged"]] == [762, 753], "kept > S for the first component in device order, and for the second"
        assert all(c["m"] <= 2 * c["S"] for c in g["comps"])
    (c,) = study("eps0-step1-oblique")["groups"][0]["comps"]
    assert (c["S"], c["m"], len(xy(study("eps0-step1-oblique")["merged"][0]))) == (764, 866, 860)


def test_brush_below_one():
    assert same_polys(study("brush0")["lines"], study("brush1")["lines"]), "radius 0 both, boxes grown by 6 or 8: the same groups here"
    assert not same_polys(study("brush-2")["lines"], study("brush1")["lines"]) and len(study("brush-2")["groups"]) == 2, "boxes grown by 2: the pair and the oblique lines part"


# ---------------------------------------------------------------- post_minlen
def test_minlen_edges():
    a, b, c = (study(f"minlen{m}") for m in (2, 0, -5))
    assert same_polys(a["lines"], b["lines"]) and same_polys(a["lines"], c["lines"]), "need = max(2, post_minlen)"
    assert len(a["merged"]) == 2 and len(run(400, 400, BY_ID["minlen2"][3], {})[3]) == 1, "the 30-px line survives only below the default"
    assert len(study("minlen_eq_path")["merged"]) == 1 and len(study("minlen_path_plus1")["merged"]) == 0
    (g,) = study("minlen_path_plus1")["groups"]
    assert len(g["comps"][0]["anchored"]) == C.TIE_PATH and g["comps"][0]["path"] == []
    assert study("minlen500")["lines"] == [] and len(study("minlen500")["lines2"]) == 6


def test_combinations_move_all_four():
    for seed in range(3):
        o = C.combo(seed)
        assert o["post_brush"] != 16 and o["post_step"] != 6.0 and o["post_eps"] != 1.28 and o["post_minlen"] != 32
        assert len(study(f"combo{seed}")["merged"]) >= 2
    assert len({C.combo(s)["post_brush"] for s in range(3)}) == 3
