"""The cases of tests/analyze_cases.py without a GPU: with the numpy double (tests/analyze_double.py) alone, every case reaches the path it is named after --
D, nseg and per of the big tables, the index each literal seed lands on, the zero-weight condition, the ties, the iteration counts around the host's look
every 8 iterations, what the filter keeps -- and hue_counts_np is the scalar hue_bucket.  tests/test_gpu_analyze_cases.py then runs the same cases on the
device."""
import os
import re

import numpy as np
import pytest

import analyze_cases as A
import analyze_double as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "golden_analyze.npz"))


def _rgb_of(keys):
    keys = np.asarray(keys, np.uint32)
    return np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], 1).astype(np.float64)


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "omnirevolve-image-processor_amd", "csrc", "analyze.hip")).read()
    assert int(re.search(r"#define AN_SEG (\d+)", src).group(1)) == A.AN_SEG
    assert re.search(r"#define AN_BINS \(1u << 24\)", src) and A.AN_BINS == 1 << 24
    assert (int(re.search(r"#define AN_MAXK (\d+)", src).group(1)), int(re.search(r"#define AN_MAX_INIT (\d+)", src).group(1))) == (A.MAXK, A.MAX_INIT)
    caps = re.findall(r"std::min<int64_t>\((\d+), cdiv\(D, 256\)\)", src)                       # the grids of k_an_hue and k_an_assign
    assert caps == [str(A.GRID_CAP)] * 2 and A.ONE_PASS == 262144
    assert int(re.search(r"const int LOOK = (\d+);", src).group(1)) == A.LOOK
    assert "const unsigned per = (nseg + 255) / 256;" in src


# ---- 1. tables past one pass of the grid and past 256 segments
@pytest.mark.parametrize("name", list(A.BIG))
def test_big_tables_reach_what_they_are_named_after(name):
    shape, d, nseg, per, npass = A.BIG[name]
    keys, counts, kept, used_all = D.color_table(A.distinct_image(name), ignore_white=False)
    assert len(keys) == kept == d == shape[0] * shape[1] and not used_all and (counts == 1).all()
    assert A.nseg_per(len(keys)) == (nseg, per) and A.passes(len(keys)) == npass


def test_big_tables_sit_on_the_thresholds():
    sizes = sorted(v[1] for v in A.BIG.values())
    assert sizes == [A.ONE_PASS, A.ONE_PASS + 1, 262656, 256 * A.AN_SEG, 256 * A.AN_SEG + 1, 562500]
    assert A.passes(A.ONE_PASS) == 1 and A.passes(A.ONE_PASS + 1) == 2
    assert A.nseg_per(256 * A.AN_SEG) == (256, 1) and A.nseg_per(256 * A.AN_SEG + 1) == (257, 2)
    # nseg = 257, per = 2: thread t owns segments 2 t and 2 t + 1, so thread 128 owns segment 256 alone and the threads above it own none
    assert [t for t in range(256) if 2 * t < 257 <= 2 * t + 1] == [128]
    assert all(A.nseg_per(d)[1] == 1 and A.passes(d) == 1 for d in (1, 121303))                  # what the suite reached before: its largest table is `noise`


# ---- 2. steered seeding
@pytest.fixture(scope="module")
def steer_table():
    keys, counts, _, _ = D.color_table(A.distinct_image(A.STEER_TABLE), ignore_white=False)
    assert len(keys) == A.STEER_D and (counts == 1).all()
    return keys, counts


@pytest.mark.parametrize("want", list(A.STEER))
def test_steered_seed_lands_on_its_index(steer_table, want):
    keys, counts = steer_table
    seed = A.STEER[want][0]
    assert D.splitmix64(seed) % A.STEER_D == want
    assert D.seed_indices(keys, counts, A.STEER_KMEANS["K"], seed, 0)[0] == want


def test_steered_indices_are_the_edges():
    nseg, per = A.nseg_per(A.STEER_D)
    assert (nseg, per) == (275, 2) and A.STEER_D - 274 * A.AN_SEG == 1348                        # a partial last segment
    assert set(A.STEER) == {0, 7, 8, A.AN_SEG - 1, A.AN_SEG, per * A.AN_SEG - 1, per * A.AN_SEG, 256 * A.AN_SEG - 1, 256 * A.AN_SEG, A.STEER_D - 1}
    owner = lambda i: (i // A.AN_SEG) // per                                                     # the thread of the segment search that owns colour i's segment
    assert owner(4095) == 0 and owner(4096) == 1 and owner(2047) == owner(2048) == 0
    assert 524288 // A.AN_SEG == 256 and 524287 // A.AN_SEG == 255                               # segment 256: beyond the 256 segments that per = 1 reads
    assert (A.STEER_D - 1) // A.AN_SEG == nseg - 1


def test_the_vectorised_search_finds_the_literals():
    found = D.first_draw_seeds(A.STEER_D, list(A.STEER))
    assert found == {w: s for w, (s, _) in A.STEER.items()}                                      # each literal is the smallest seed below 2^23
    x = np.array([0, 1, 42, 2 ** 63 + 5, 2 ** 64 - 1], np.uint64)
    assert D.splitmix64_np(x).tolist() == [D.splitmix64(int(v)) for v in x]


@pytest.mark.parametrize("keys,K,seed,hit", A.ZERO_WEIGHT)
def test_zero_weight_directly_behind_the_target(keys, K, seed, hit):
    keys = np.array(keys, np.uint32); counts = np.ones(len(keys), np.int64)
    assert hit in A.zero_weight_hits(keys, counts, K, seed)
    step, c = hit
    t, pre, chosen, pick = A.seed_trace(keys, counts, K, seed)[step]
    w = np.diff(np.concatenate([[0], pre]))
    assert c in chosen and w[c] == 0 and t == pre[c] and pick > c and w[pick] > 0                # the prefix of c equals the target: c must be stepped over
    assert pick == min(i for i in range(c + 1, len(keys)) if w[i] > 0)
    assert D.seed_indices(keys, counts, K, seed, 0)[step] == pick


def test_zero_weight_pins_cover_both_ends_of_the_table():
    assert any(hit[1] == 0 for _, _, _, hit in A.ZERO_WEIGHT) and len(A.ZERO_WEIGHT) >= 4 and len({tuple(k) for k, _, _, _ in A.ZERO_WEIGHT}) >= 2
    for keys, K, seed, step in A.ZERO_TAIL:
        keys = np.array(keys, np.uint32); counts = np.ones(len(keys), np.int64)
        assert step in A.zero_tail_hits(keys, counts, K, seed)
        t, pre, chosen, pick = A.seed_trace(keys, counts, K, seed)[step]
        w = np.diff(np.concatenate([[0], pre]))
        last = len(keys) - 1
        assert last in chosen and w[last] == 0 and t == pre[-1] - 1 and pick == max(i for i in range(last) if w[i] > 0)


def test_zero_weight_search_finds_the_pinned_seeds():
    assert sorted(A.search_zero_weight(A.ZERO_KEYS, 4, range(2000))) == [118, 1092, 1658, 1673, 1923, 1984]
    assert 688 in A.search_zero_weight(A.ZERO_KEYS, 4, range(600, 700), A.zero_tail_hits)


# ---- 3. Lloyd at its edges
@pytest.mark.parametrize("name", list(A.TIES))
def test_ties_go_to_the_lower_index(name):
    keys, mid, seeds = A.TIES[name]
    keys = np.array(keys, np.uint32); counts = np.ones(3, np.int64)
    orders = set()
    for seed, want in seeds.items():
        ch = D.seed_indices(keys, counts, 2, seed, 0)
        assert ch == want and mid not in ch
        orders.add(tuple(ch))
        cen = _rgb_of(keys)[ch]
        d = ((_rgb_of(keys)[mid] - cen) ** 2).sum(1)
        assert d[0] == d[1] > 0                                                                   # small integers: exact in any order
        c, n, sums, it = D.lloyd(keys, counts, cen, 1)
        assert n.tolist() == [2, 1] and sums[0].tolist() == (_rgb_of(keys)[mid] + cen[0]).astype(np.int64).tolist()
    assert len(orders) == 2                                                                       # both orders: the middle colour goes with a different neighbour
    if name == "blue_against_red_green":
        m, c0, c1 = _rgb_of(keys)
        assert ((m - c0) ** 2).tolist() == [0, 0, 25] and ((m - c1) ** 2).tolist() == [9, 16, 0]


@pytest.fixture(scope="module")
def look_runs():
    out = {}
    for name, (img, K, seed, _) in A.LOOK_CASES.items():
        keys, counts, _, _ = D.color_table(G[f"img_{img}"])
        out[name] = D.kmeans(keys, counts, K, n_init=2, max_iter=300, seed=seed)
    return out


@pytest.mark.parametrize("name", list(A.LOOK_CASES))
def test_look_cases_freeze_one_init_while_the_other_passes_two_looks(look_runs, name):
    want = A.LOOK_CASES[name][3]
    it = look_runs[name][3].tolist()
    assert it == want
    assert min(it) < A.LOOK and max(it) > 2 * A.LOOK + 1                                          # frozen before the first look; running past the looks at 8 and 16
    assert {A.LOOK - 1, A.LOOK, A.LOOK + 1, 2 * A.LOOK, 2 * A.LOOK + 1, 1} <= set(A.LOOK_MAX_ITER) and max(A.LOOK_MAX_ITER) > max(it)
    assert (it[0] > it[1]) == (name == "long_then_short")


def test_limits_table_holds_both_maxima():
    keys, counts, _, _ = D.color_table(A.limits_image())
    assert len(keys) == 40 >= A.MAXK
    cen, n, sums, it = D.kmeans(keys, counts, A.MAXK, n_init=A.MAX_INIT, max_iter=20)
    assert cen.shape == (64, 32, 3) and (n.sum(1) == counts.sum()).all()


def test_heavy_weights():
    keys, counts, kept, _ = D.color_table(A.heavy_image(), ignore_white=False)
    assert len(keys) == 5 and kept == 1 << 20 and counts[0] == 1 << 19 and counts[-1] == (1 << 19) - 3 and sorted(counts.tolist())[:3] == [1, 1, 1]
    tr = A.seed_trace(keys, counts, 2, 42)
    assert tr[0][3] in (0, 4) and int(tr[1][1][-1]) > 5 * 10 ** 5 * 195075 * 0.99                 # the second draw's total: half a million pixels at 3 * 255^2
    cen, n, sums, it = D.kmeans(keys, counts, 2, n_init=2, max_iter=10)
    assert sums.max() > 10 ** 8


@pytest.mark.parametrize("name", list(A.EMPTY_CLUSTER))
def test_empty_cluster_cases_empty_a_cluster(name):
    """the n > 0 else-branch of k_an_update: an iteration leaves a cluster without a colour and the cluster keeps its centre"""
    keys, counts, K, seed, it, k, n_final = A.EMPTY_CLUSTER[name]
    keys = np.array(keys, np.uint32); counts = np.array(counts, np.int64)
    assert A.lloyd_empty(keys, counts, _rgb_of(keys)[D.seed_indices(keys, counts, K, seed, 0)]) == it
    before = D.kmeans(keys, counts, K, n_init=1, max_iter=it - 1, seed=seed)
    at = D.kmeans(keys, counts, K, n_init=1, max_iter=it, seed=seed)
    assert before[1][0, k] > 0 and at[1][0, k] == 0 and (at[1][0] == 0).sum() == 1 and at[2][0, k].tolist() == [0, 0, 0]
    assert at[0][0, k].tobytes() == before[0][0, k].tobytes()                                     # the centre is kept
    final = D.kmeans(keys, counts, K, n_init=1, max_iter=300, seed=seed)
    assert final[1][0].tolist() == n_final and final[3][0] > it and (n_final[k] == 0) == (name == "stays_empty")
    assert {it - 1, it, it + 1} <= set(A.EMPTY_MAX_ITER)


def test_the_empty_cluster_search_reports_a_cluster_without_a_colour():
    keys = np.array([0, 1, 2, 200], np.uint32)
    assert A.lloyd_empty(keys, np.ones(4, np.int64), [[0, 0, 0.0], [0, 0, 1.0], [0, 0, 0.4]]) == 1
    assert A.lloyd_empty(keys, np.ones(4, np.int64), [[0, 0, 0.0], [0, 0, 1.0], [0, 0, 200.0]]) == 0
    assert A.search_empty_cluster(100) == []                                                      # rare: two tables in the first 30 000 (EMPTY_CLUSTER)


# ---- 4. the table kernels
def test_edge_keys_and_the_filter():
    img = A.edge_image()
    keys, counts, kept, used_all = D.color_table(img, ignore_white=False)
    assert keys.tolist() == A.EDGE_KEYS and counts.tolist() == A.EDGE_COUNTS and len(set(A.EDGE_COUNTS)) == len(A.EDGE_KEYS)
    white = A.is_white(A.EDGE_KEYS)
    assert white.tolist() == [False] * 9 + [True]                                                 # 2^24 - 4097 = (255, 239, 255), 2^24 - 4096 = (255, 240, 0)
    keys, counts, kept, used_all = D.color_table(img)
    assert not used_all and keys.tolist() == [k for k, w in zip(A.EDGE_KEYS, white) if not w] and kept == sum(A.EDGE_COUNTS[:-1])
    assert {k % 16 for k in A.EDGE_KEYS} >= {0, 15} and {k % 4096 for k in A.EDGE_KEYS} >= {0, 4095}


def test_every_colour_image_is_a_permutation():
    img = A.every_colour_image().reshape(-1, 3).astype(np.uint32)
    assert (np.bincount(img[:, 0] << 16 | img[:, 1] << 8 | img[:, 2], minlength=1 << 24) == 1).all() and len(img) == A.AN_BINS
    assert int(A.is_white(np.arange(1 << 24)).sum()) == 16 ** 3


def test_filter_decides_at_equality():
    keys, counts, kept, used_all = D.color_table(A.filter_image(100))
    assert (kept, used_all) == (100, False) and not A.is_white(keys).any() and len(keys) == 2
    keys, counts, kept, used_all = D.color_table(A.filter_image(99))
    assert (kept, used_all) == (256, True) and A.is_white(keys).any() and counts[A.is_white(keys)].sum() == 157


@pytest.mark.parametrize("thr", list(A.THRESHOLDS))
def test_thresholds(thr):
    img = A.threshold_image()
    want = sorted(r << 16 | g << 8 | b for r, g, b in A.THRESHOLDS[thr])
    keys, counts, kept, used_all = D.color_table(img, white_threshold=thr, min_kept=1)
    if want:
        assert keys.tolist() == want and not used_all
    else:
        assert used_all and len(keys) == len(A.THRESHOLD_COLOURS)                                 # nothing is non-white: 0 < 1, every pixel is kept
        assert len(D.color_table(img, white_threshold=thr, min_kept=0)[0]) == 0                   # 0 < 0 is false: the filter holds and keeps nothing


def test_empty_table():
    keys, counts, kept, used_all = D.color_table(A.all_white_image(), min_kept=0)
    assert len(keys) == 0 and kept == 0 and not used_all
    assert D.hue_counts(keys, counts).tolist() == D.hue_counts_np(keys, counts).tolist() == [0] * 11
    with pytest.raises(ValueError, match="fewer"):
        D.kmeans(keys, counts, 2)


def test_wave_merging_images():
    assert 1001 * 1003 == 1004003 and 1004003 % 4 == 3 and 1003 * 1000 % 4 == 0
    assert A.keys_per_wave_slot(A.one_colour_tail()) == [1]
    assert 129 * 67 % 4 == 3
    assert max(A.keys_per_wave_slot(A.two_colour_rows())) == 2                                    # never a third key in a wave: no lane is left for the single add
    assert max(A.keys_per_wave_slot(A.three_colour_rows())) == 3


# ---- 5. hue_counts_np is the scalar hue_bucket
def _scalar_buckets(keys):
    ix = {n: i for i, n in enumerate(D.HUE_KEYS)}
    return [ix[D.hue_bucket(k >> 16, (k >> 8) & 255, k & 255)] for k in keys.tolist()]


def test_hue_np_on_the_hand_checked_list():
    keys = np.array([r << 16 | g << 8 | b for (r, g, b), _, _ in D.HUE_LIST], np.uint32)
    assert [D.HUE_KEYS[i] for i in D.hue_buckets_np(keys)] == [bucket for _, _, bucket in D.HUE_LIST]


def test_hue_np_on_a_grid_of_the_cube():
    ch = np.array(sorted(set(range(0, 256, 5)) | {49, 50, 255}), np.uint32)
    keys = (ch[:, None, None] << 16 | ch[None, :, None] << 8 | ch[None, None, :]).ravel()
    assert len(keys) == 53 ** 3 and D.hue_buckets_np(keys).tolist() == _scalar_buckets(keys)


def test_hue_np_on_random_colours():
    rng = np.random.default_rng(11)
    keys = rng.integers(0, 1 << 24, 200000).astype(np.uint32)
    assert D.hue_buckets_np(keys).tolist() == _scalar_buckets(keys)
    u, c = np.unique(keys, return_counts=True); c = c * rng.integers(1, 10 ** 6, len(c))
    assert D.hue_counts_np(u, c).tolist() == D.hue_counts(u, c).tolist()
