"""analyze_colors without a GPU: the numpy double of the device side (tests/analyze_double.py) against what scikit-learn's KMeans found
(tests/golden/golden_analyze.npz, made by tests/golden/make_golden_analyze.py), and the host module orip/analyze.py -- palette, recommendation, report
file.  Lab here is the oracle's BGR2LAB restatement; on the product path it is Device.lab_of_rgb (tests/test_gpu_analyze.py compares the two)."""
import json
import os

import numpy as np
import pytest

import analyze_double as D
from analyze_double import DoubleDevice, HUE_LIST, lab_cpu
from orip import analyze as AN
from orip import colors as PC

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_analyze.npz"))
CASES = [str(c) for c in G["cases"]]


def lab_identity(rgb):
    """"Lab" := R, G, B, so that distances in the branch tests can be checked by hand"""
    return np.asarray(rgb, np.uint8).reshape(-1, 3)


# ---- 1. the double against sklearn's recorded optimum
def test_fixture_holds_asserted_cases_for_every_image():
    assert len(CASES) >= 6 and {c.split(":")[0] for c in CASES} == {"a", "b", "c"}
    for c in CASES:
        nm, K = c.split(":")
        inert = G[f"K_{nm}_{K}_inertia"]
        assert len(inert) == 20 and inert.max() / inert.min() - 1.0 < 1e-6          # the fixture condition: the optimum is unambiguous for sklearn itself


@pytest.mark.parametrize("case", CASES)
def test_double_reaches_sklearns_optimum(case):
    """inertia of our centres over every kept pixel, float64, at most sklearn's largest recorded inertia times (1 + 1e-9): the measure is sklearn's own
    spread over 20 seeds, the 1e-9 covers float64 summation order over <= 5e4 terms"""
    nm, K = case.split(":"); K = int(K)
    img = G[f"img_{nm}"]
    keys, counts, kept, used_all = D.color_table(img)
    px, _ = D.kept_pixels(img)
    assert kept == len(px) <= 50000 and not used_all
    cen, n, sums, _ = D.kmeans(keys, counts, K)
    b = D.best_init(keys, counts, n, sums)
    assert b == AN.best_init(n, sums)                                               # the host's exact choice is the double's
    ours, theirs = D.pixel_inertia(px, cen[b]), float(G[f"K_{nm}_{K}_inertia"].max())
    print(f"{case}: ours {ours!r}, sklearn max {theirs!r}, min {float(G[f'K_{nm}_{K}_inertia'].min())!r}")
    assert ours <= theirs * (1 + 1e-9)
    # the same recommendation from our clusters and from sklearn's recorded cluster list
    for boost in (True, False):
        a = AN.ColorAnalyzer(AN.Palette(None, lab_cpu)); a.set_clusters(cen[b], n[b])
        s = AN.ColorAnalyzer(AN.Palette(None, lab_cpu)); s.set_dominant(G[f"K_{nm}_{K}_rgb"], G[f"K_{nm}_{K}_pct"])
        assert [r[0] for r in a.recommend_colors(4, boost)] == [r[0] for r in s.recommend_colors(4, boost)]


def test_seeding_is_the_stated_stream():
    assert D.splitmix64(0) == 0xE220A8397B1DCDAF and D.splitmix64(1) == 0x910A2DEC89025CC1      # the published first outputs of splitmix64 for these states
    keys = np.array([0x000000, 0x0000FF, 0x00FF00, 0xFF0000], np.uint32); counts = np.array([5, 1, 1, 1], np.int64)
    ch = D.seed_indices(keys, counts, 3, 42, 0)
    t0 = D.splitmix64(42 ^ 0) % 8
    assert ch[0] == (0 if t0 < 5 else t0 - 4) and len(set(ch)) == 3                               # a chosen colour has weight 0 afterwards


# ---- 2. Palette
def test_palette_distance_grouping_and_order():
    p = AN.Palette({"a": (10, 10, 10), "b": (13, 14, 10), "c": (10, 10, 40), "d": (13, 14, 10), "far": (200, 0, 0)}, lab_identity)
    assert p.find_closest((10, 10, 10), 3) == [("a", 0.0), ("b", 5.0), ("d", 5.0)]              # equal distances: palette order
    assert p.find_closest((255, 0, 0), 1) == [("far", 55.0)]                                      # integers, no uint8 wrap-around: 255 - 200, not 55 mod 256 by luck
    assert p.find_closest((0, 0, 0), 1)[0][1] == pytest.approx(np.sqrt(300.0))
    assert p.get_color_group("a", 5) == ["a", "b", "d"] and p.get_color_group("a", 4.99) == ["a"] and p.get_color_group("a", 30) == ["a", "b", "c", "d"]
    assert p.get_color_group("far", 1000) == ["a", "b", "c", "d", "far"]
    q = AN.Palette({"lo": (2, 0, 0), "hi": (250, 0, 0)}, lab_identity)
    assert q.find_closest((250, 0, 0), 2) == [("hi", 0.0), ("lo", 248.0)]                         # a wrapped difference would be 8
    with pytest.raises(RuntimeError, match="lab_of_rgb"):
        AN.Palette().find_closest((1, 2, 3))
    with pytest.raises(ValueError):
        AN.Palette({"x": (1, 2, 300)})
    d = AN.Palette(None, lab_cpu)
    assert len(d.colors) == len(AN.DEFAULT_MARKERS) >= 16 and "Carioca" in AN.Palette.__doc__ and d.find_closest((20, 20, 20))[0] == ("black", 0.0)
    lab = lab_cpu([(255, 255, 255), (0, 0, 0)])
    assert lab.tolist() == [[255, 128, 128], [0, 128, 128]]


def test_palette_load_both_layouts(tmp_path):
    a = tmp_path / "a.json"; a.write_text(json.dumps({"palette": [{"rgb": [1, 2, 3]}, {"name": "x", "rgb": [200, 100, 50]}]}))
    p = AN.Palette.load(str(a), lab_identity)
    assert p.colors == {"color_0": (1, 2, 3), "x": (200, 100, 50)}
    rgb, names = PC.palette_from_json(str(a))                                                     # the same names as the loader process_colors uses
    assert names == list(p.colors) and rgb.tolist() == [list(v) for v in p.colors.values()]
    b = tmp_path / "b.json"; b.write_text(json.dumps(PC.palette_dump(np.array([[9, 8, 7], [6, 5, 4]], np.uint8), ["n0"])))
    assert AN.Palette.load(str(b), lab_identity).colors == {"n0": (9, 8, 7), "color_1": (6, 5, 4)}
    c = tmp_path / "c.json"; c.write_text(json.dumps({"something": 1}))
    with pytest.raises(ValueError, match="Unsupported palette JSON"):
        AN.Palette.load(str(c))


# ---- 3. recommend_colors branches on hand-made cluster lists ("Lab" = RGB)
def _analyzer(colors, doms):
    a = AN.ColorAnalyzer(AN.Palette(colors, lab_identity))
    a.set_dominant([d[0] for d in doms], [d[1] for d in doms])
    return a


def test_recommend_penalty_for_far_clusters():
    pal = {"dark": (0, 0, 0), "light": (200, 200, 200)}
    a = _analyzer(pal, [((0, 0, 51), 60.0), ((200, 200, 200), 40.0)])                             # distance 51 > 50: 60 * 0.5 = 30 < 40
    assert a.dominant_colors[0]["distance"] == 51.0
    assert sorted(a.recommend_colors(2, False), key=lambda r: -r[1]) == [("light", 40.0), ("dark", 30.0)]
    b = _analyzer(pal, [((0, 0, 50), 60.0), ((200, 200, 200), 40.0)])                             # distance 50 is not > 50
    assert dict(b.recommend_colors(2, False)) == {"dark": 60.0, "light": 40.0}
    assert [r[0] for r in b.recommend_colors(2, False)] == ["light", "dark"]                      # light -> dark
    with pytest.raises(ValueError, match="analyze"):
        AN.ColorAnalyzer(AN.Palette(pal, lab_identity)).recommend_colors()


def test_recommend_boost_spreads_to_the_group():
    pal = {"a": (100, 0, 0), "b": (100, 40, 0), "c": (100, 81, 0), "z": (0, 0, 200)}             # a-b 40 (in the group), a-c 81, b-c 41 (not)
    a = _analyzer(pal, [((100, 0, 0), 50.0), ((0, 0, 200), 50.0)])
    assert dict(a.recommend_colors(4, True)) == {"a": 50.0, "b": 15.0, "z": 50.0}
    assert dict(a.recommend_colors(4, False)) == {"a": 50.0, "z": 50.0}
    both = _analyzer(pal, [((100, 0, 0), 50.0), ((100, 40, 0), 20.0)])                            # a and b boost each other
    assert dict(both.recommend_colors(4, True)) == {"a": 50.0 + 20.0 * 0.3, "b": 20.0 + 50.0 * 0.3}


def test_recommend_dedup_wraps_as_written():
    """:233 subtracts uint8 arrays: candidate - selected wraps modulo 256.  10 - 250 -> 16 (< 30: dropped, true distance 240); 250 - 10 -> 240 (kept)."""
    pal = {"hi": (250, 0, 0), "lo": (10, 0, 0), "other": (0, 200, 0)}
    a = _analyzer(pal, [((250, 0, 0), 50.0), ((10, 0, 0), 30.0), ((0, 200, 0), 20.0)])            # hi is selected first, lo is the candidate
    assert [r[0] for r in a.recommend_colors(3, False)] == ["hi", "other"]
    b = _analyzer(pal, [((10, 0, 0), 50.0), ((250, 0, 0), 30.0), ((0, 200, 0), 20.0)])            # lo first: 250 - 10 = 240, both stay
    assert sorted(r[0] for r in b.recommend_colors(3, False)) == ["hi", "lo", "other"]
    near = _analyzer({"p": (100, 100, 100), "q": (110, 110, 110), "r": (0, 0, 0)}, [((100, 100, 100), 50.0), ((110, 110, 110), 30.0), ((0, 0, 0), 20.0)])
    assert [r[0] for r in near.recommend_colors(3, False)] == ["p", "r"]                          # 17.3 < 30 without any wrap


def test_recommend_more_colours_than_candidates_and_the_12_cluster_cap():
    pal = {"a": (0, 0, 0), "b": (255, 255, 255)}
    a = _analyzer(pal, [((0, 0, 0), 70.0), ((255, 255, 255), 30.0)])
    assert a.recommend_colors(10, False) == [("b", 30.0), ("a", 70.0)]
    many = _analyzer(pal, [((0, 0, 0), 5.0)] * 12 + [((255, 255, 255), 40.0)])                    # :196 reads the first 12 clusters only
    assert many.recommend_colors(4, False) == [("a", 60.0)]


def test_set_clusters_truncates_and_orders_stably():
    a = AN.ColorAnalyzer(AN.Palette({"k": (0, 0, 0)}, lab_identity))
    a.set_clusters([[10.99, 0.5, 3.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]], [5, 10, 5])
    assert [d["rgb"] for d in a.dominant_colors] == [(1, 1, 1), (10, 0, 3), (2, 2, 2)]            # astype(int) truncates; equal sizes keep their order
    assert [d["percentage"] for d in a.dominant_colors] == [50.0, 25.0, 25.0]


# ---- 4. the white-threshold fallback
def test_white_fallback_below_100_pixels(capsys):
    img = np.full((40, 150, 3), 250, np.uint8)
    img[0, :99] = (10, 200, 30)
    keys, counts, kept, used_all = D.color_table(img)
    assert used_all and kept == 6000 and dict(zip(keys.tolist(), counts.tolist())) == {0x0AC81E: 99, 0xFAFAFA: 5901}
    img[0, 99] = (239, 250, 250)                                                                   # one channel below 240 is enough (:60)
    keys, counts, kept, used_all = D.color_table(img)
    assert not used_all and kept == 100 and dict(zip(keys.tolist(), counts.tolist())) == {0x0AC81E: 99, 0xEFFAFA: 1}
    assert D.color_table(img, ignore_white=False)[2:] == (6000, False)
    img[0, 99] = 250
    a = AN.ColorAnalyzer(AN.Palette(None, lab_cpu))
    res = a.analyze(DoubleDevice(img), n_clusters=2, n_init=2)
    assert "Warning: Image is mostly white, using all pixels" in capsys.readouterr().out and a.used_all_pixels
    assert res["analyzed_pixels"] == res["total_pixels"] == 6000 and res["image_size"] == (150, 40)
    assert [round(d["percentage"], 2) for d in res["dominant_colors"]] == [98.35, 1.65] and res["dominant_colors"][0]["rgb"] == (250, 250, 250)


# ---- 5. hue buckets on the hand-checked colour list (analyze_double.HUE_LIST)
def test_hue_buckets_on_a_hand_checked_list():
    for rgb, hsv, bucket in HUE_LIST:
        assert D.hsv8(*rgb) == hsv and D.hue_bucket(*rgb) == bucket, (rgb, D.hsv8(*rgb), D.hue_bucket(*rgb))
    rgb = np.array([c[0] for c in HUE_LIST], np.uint8)
    img = np.repeat(rgb[None], 3, axis=0)                                                          # every colour three times
    keys, counts, kept, _ = D.color_table(img, ignore_white=False)
    want = {k: 0 for k in AN.HUE_KEYS}
    for _, _, bucket in HUE_LIST:
        want[bucket] += 3
    assert D.HUE_KEYS == AN.HUE_KEYS and D.hue_counts(keys, counts).tolist() == [want[k] for k in AN.HUE_KEYS] and kept == 3 * len(HUE_LIST)
    assert want == {"red": 12, "orange": 18, "yellow": 6, "green": 6, "cyan": 6, "blue": 6, "purple": 9, "pink": 9, "brown": 6, "gray": 6, "black": 6}
    a = AN.ColorAnalyzer(AN.Palette(None, lab_cpu)); a.set_hue_counts(D.hue_counts(keys, counts))
    assert a.color_histogram["red"] == 12 / 90 * 100 and abs(sum(a.color_histogram.values()) - 100) < 1e-9


# ---- 6. the report file
def test_colors_json_round_trips_through_process_colors_loader(tmp_path):
    img = G["img_b"]
    a = AN.ColorAnalyzer(AN.Palette(None, lab_cpu))
    a.analyze(DoubleDevice(img), n_clusters=4)
    rec = a.recommend_colors(3)
    assert len(rec) == 3
    path = tmp_path / "img_colors.json"
    path.write_text(json.dumps(AN.recommendations_json("img.png", a.palette, rec), indent=2))
    data = json.loads(path.read_text())
    assert data["image"] == "img.png" and [sorted(it) for it in data["recommended_colors"]] == [["coverage", "name", "position", "rgb"]] * 3
    assert [it["position"] for it in data["recommended_colors"]] == [1, 2, 3]
    rgb, names = PC.palette_from_json(str(path))
    assert names == [r[0] for r in rec] and rgb.tolist() == [list(a.palette.colors[r[0]]) for r in rec]
    lum = [np.mean(a.palette.colors[n]) for n in names]
    assert lum == sorted(lum, reverse=True)                                                        # light -> dark
