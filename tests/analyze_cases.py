"""TEST INFRASTRUCTURE: named inputs for analyze_colors (csrc/analyze.hip) at the sizes and draws its launch caps, its two-level seeding search and its host
loop turn on, with the literal seeds that steer them.  tests/test_analyze_cases_host.py shows with the numpy double (tests/analyze_double.py) alone that every
case reaches what it is named after; tests/test_gpu_analyze_cases.py runs them on the device against the double, bit for bit.  No GPU import, no test here.

The constants below restate the kernel's launch geometry.  The host test computes nseg and per from them for every table, so a change of AN_SEG or of a grid
cap that is mirrored here makes the case names fail instead of silently no longer reaching the paths; a change that is not mirrored is caught by
test_constants_are_the_kernels, which reads them out of the source."""
import functools

import numpy as np

import analyze_double as D

AN_SEG = 2048                      # colours per segment of the seeding
AN_BINS = 1 << 24
GRID_CAP = 1024                    # k_an_hue and k_an_assign: min(GRID_CAP, cdiv(D, 256)) blocks of 256 threads
ONE_PASS = GRID_CAP * 256          # 262 144: the largest table a single pass covers
LOOK = 8                           # the host reads the done flags every LOOK iterations
MAXK, MAX_INIT = 32, 64


def nseg_per(d):
    """(segments of the seeding, segments per thread of k_an_seed_pick)"""
    nseg = (d + AN_SEG - 1) // AN_SEG
    return nseg, (nseg + 255) // 256


def passes(d):
    """rounds of the grid-stride loops of k_an_hue / k_an_assign"""
    blocks = min(GRID_CAP, (d + 255) // 256)
    return (d + blocks * 256 - 1) // (blocks * 256)


def key_image(keys, shape=None):
    """RGB image holding `keys` in this order"""
    k = np.asarray(keys, np.uint32)
    img = np.stack([k >> 16, (k >> 8) & 255, k & 255], -1).astype(np.uint8)
    return img.reshape((1, -1, 3) if shape is None else tuple(shape) + (3,))


def weighted_image(keys, counts):
    """one row holding keys[i] counts[i] times"""
    return key_image(np.repeat(np.asarray(keys, np.uint32), np.asarray(counts, np.int64)))


# ---- 1. every pixel its own colour (run with ignore_white=False: D = the pixel count)
BIG = {                            # name: (shape, D, nseg, per, passes)
    "one_pass_262144": ((512, 512), 262144, 128, 1, 1),
    "second_pass_by_one_262145": ((1, 262145), 262145, 129, 1, 2),
    "second_pass_262656": ((512, 513), 262656, 129, 1, 2),
    "nseg_256_524288": ((1, 524288), 524288, 256, 1, 2),
    "nseg_257_524289": ((1, 524289), 524289, 257, 2, 3),
    "nseg_275_562500": ((750, 750), 562500, 275, 2, 3),
}
BIG_KMEANS = dict(K=3, n_init=2, max_iter=6, seed=42)


@functools.lru_cache(maxsize=None)
def distinct_image(name):
    shape = BIG[name][0]
    n = shape[0] * shape[1]
    return key_image(np.random.default_rng(n).choice(1 << 24, n, replace=False), shape)


# ---- 2. steered seeding.  On STEER_TABLE every count is 1, so the first draw of init 0, splitmix64(seed) % D, is the table index of the first centre.
STEER_TABLE = "nseg_275_562500"
STEER_D = 562500
STEER = {                          # wanted index: (seed, what the index is)
    0: (595145, "colour 0"),
    7: (331777, "the last colour of thread 0"),
    8: (124611, "the first colour of thread 1"),
    2047: (2440854, "the last colour of segment 0"),
    2048: (278185, "the first colour of segment 1, still thread 0 of the segment search (per = 2)"),
    4095: (1679172, "the last colour of thread 0's second segment"),
    4096: (148770, "the first colour of thread 1's first segment"),
    524287: (512217, "the last colour of segment 255"),
    524288: (16355, "the first colour of segment 256, which a search with per = 1 never looks at"),
    562499: (805922, "colour D - 1, in the partial last segment (1348 colours)"),
}
STEER_KMEANS = dict(K=3, n_init=1, max_iter=3)


def seed_trace(keys, counts, K, seed, init=0):
    """analyze_double.seed_indices, step by step -> [(target, inclusive prefix sums, indices chosen before the step, index picked)]"""
    rgb = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], 1).astype(np.int64)
    cnt = np.asarray(counts, np.int64)
    mind2, chosen, out = None, [], []
    for step in range(K):
        w = cnt if step == 0 else cnt * mind2
        pre = np.cumsum(w)
        t = D.splitmix64((seed ^ ((init << 32) + step)) & D.M64) % int(pre[-1])
        i = int(np.searchsorted(pre, t, side="right"))
        out.append((t, pre, list(chosen), i))
        chosen.append(i)
        d2 = ((rgb - rgb[i]) ** 2).sum(1)
        mind2 = d2 if mind2 is None else np.minimum(mind2, d2)
    return out


def zero_weight_hits(keys, counts, K, seed, init=0):
    """[(step, c)]: at `step` the target equals the sum of the weights in front of colour c, and c was chosen before (its weight is 0).  The prefix sum of
    c then EQUALS the target, so the first prefix sum above it belongs to a later colour: the search has to step over c."""
    hits = []
    for step, (t, pre, chosen, _) in enumerate(seed_trace(keys, counts, K, seed, init)):
        for c in chosen:
            if t == (int(pre[c - 1]) if c else 0):
                hits.append((step, c))
    return hits


def zero_tail_hits(keys, counts, K, seed, init=0):
    """[step]: the last colour of the table was chosen before `step` and the target is total - 1, the largest there is.  (The target can never equal the sum
    in front of the last colour, which is the total: this is the nearest a draw comes to a zero weight at the end of the table.)"""
    return [step for step, (t, pre, chosen, _) in enumerate(seed_trace(keys, counts, K, seed, init)) if len(keys) - 1 in chosen and t == int(pre[-1]) - 1]


def search_zero_weight(keys, K, seeds, fn=zero_weight_hits):
    """the seeds of `seeds` with a hit, counts all 1 -> {seed: hits}"""
    counts = np.ones(len(keys), np.int64)
    keys = np.asarray(keys, np.uint32)
    return {s: h for s in seeds for h in [fn(keys, counts, K, s)] if h}


ZERO_KEYS = [350, 734, 742, 969, 3282, 3319]          # six colours, counts 1, K = 4: search_zero_weight finds 56 of the seeds 0 .. 19 999
ZERO_KEYS_8 = [0x0A0A0A, 0x0A0A0C, 0x0A0C0A, 0x0C0A0A, 0x0C0C0C, 0x0E0A0B, 0x0E0E0E, 0x101010]      # eight close colours, K = 5: small totals, many hits
ZERO_WEIGHT = [                    # (keys, K, seed, (step, c)): found with search_zero_weight
    (ZERO_KEYS, 4, 118, (3, 0)),   # colours 0 and 1 are both chosen and the target is 0: two zero weights at the head of the table
    (ZERO_KEYS, 4, 1673, (2, 0)),  # the first colour of the table, at step 2
    (ZERO_KEYS, 4, 1984, (3, 3)),
    (ZERO_KEYS, 4, 3255, (3, 4)),
    (ZERO_KEYS_8, 5, 26, (4, 6)),
    (ZERO_KEYS_8, 5, 20, (4, 3)),  # colours 3 and 4 are both chosen: two zero weights in a row inside the table
]
ZERO_TAIL = [                      # (keys, K, seed, step): found with search_zero_weight(..., fn=zero_tail_hits); the zero weight is the last colour of the table
    (ZERO_KEYS, 4, 688, 3),
    (ZERO_KEYS_8, 5, 5, 3),
]


# ---- 3. Lloyd at its edges
TIES = {                           # name: (keys, table index of the equidistant colour, {seed: the two seeded table indices}); counts 1, K = 2
    "red_axis": ([0 << 16, 1 << 16, 2 << 16], 1, {1: [2, 0], 5: [2, 0], 6: [2, 0], 7: [0, 2], 11: [0, 2]}),
    # (0, 0, 0) is 25 away from (0, 0, 5) through blue alone and 9 + 16 away from (3, 4, 0) through red and green
    "blue_against_red_green": ([0x000000, 0x000005, 0x030400], 0, {0: [1, 2], 5: [2, 1]}),
}

LOOK_CASES = {                     # name: (fixture image, K, seed, iterations of the two inits without a limit)
    "long_then_short": ("a", 5, 9, [20, 3]),
    "short_then_long": ("a", 6, 6, [4, 20]),
}
LOOK_MAX_ITER = [1, 7, 8, 9, 16, 17, 300]


def limits_image():
    """40 distinct non-white colours on 23 x 31 pixels"""
    rng = np.random.default_rng(40)
    pal = np.stack([np.arange(40) * 5 + 2, rng.integers(0, 200, 40), rng.integers(0, 200, 40)], 1).astype(np.uint8)
    idx = rng.integers(0, 40, (23, 31)); idx.flat[:40] = np.arange(40)
    return pal[idx]


HEAVY_STRAYS = [(17, 130, 201), (254, 3, 99), (128, 128, 127)]


def heavy_image():
    """1024 x 1024: the upper half black, the lower half white but for three stray pixels"""
    img = np.zeros((1024, 1024, 3), np.uint8)
    img[512:] = 255
    for i, c in enumerate(HEAVY_STRAYS):
        img[600 + 100 * i, 37 + 300 * i] = c
    return img


def lloyd_empty(keys, counts, centres, max_iter=100):
    """analyze_double.lloyd's loop, asking only: does any iteration leave a cluster without a colour?  -> the first such iteration, or 0"""
    ch = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], 1).astype(np.int64)
    r, g, b = (ch[:, j].astype(np.float64) for j in range(3))
    cnt = np.asarray(counts, np.int64)
    c = np.array(centres, np.float64)
    K = len(c)
    labels = None
    for it in range(1, max_iter + 1):
        d = np.stack([((r - c[k, 0]) ** 2 + (g - c[k, 1]) ** 2) + (b - c[k, 2]) ** 2 for k in range(K)], 1)
        new = np.argmin(d, axis=1)
        n = np.bincount(new, weights=None, minlength=K)
        if (n == 0).any():
            return it
        if labels is not None and np.array_equal(new, labels):
            return 0
        labels = new
        nw = np.bincount(new, cnt, K)
        for j in range(3):
            c[:, j] = np.bincount(new, cnt * ch[:, j], K) / nw
    return 0


def search_empty_cluster(tables, rng_seed=0, spread=(256, 40, 8)):
    """`tables` random weighted tables (8 - 40 colours, K 3 - 6, counts 1 - 1000, the colours drawn from a cube of side spread[i % 3], seeded as the product
    seeds them) -> [(keys, counts, K, seed, iteration)] of those in which Lloyd empties a cluster"""
    rng = np.random.default_rng(rng_seed)
    found = []
    for i in range(tables):
        d, K, side = int(rng.integers(8, 41)), int(rng.integers(3, 7)), spread[i % len(spread)]
        keys = np.unique((rng.integers(0, side, d).astype(np.uint32) << 16) | (rng.integers(0, side, d).astype(np.uint32) << 8) | rng.integers(0, side, d).astype(np.uint32))
        if len(keys) < K:
            continue
        counts = rng.integers(1, 1001, len(keys)).astype(np.int64)
        if i % 2:
            counts[rng.integers(0, len(keys))] = 10 ** 6            # one colour that outweighs the rest
        seed = int(rng.integers(0, 1 << 30))
        rgb = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], 1).astype(np.float64)
        it = lloyd_empty(keys, counts, rgb[D.seed_indices(keys, counts, K, seed, 0)])
        if it:
            found.append((keys, counts, K, seed, it))
    return found


# search_empty_cluster(5000, rng_seed=c) for c = 0, 1, ... found nothing in the first 25 000 tables and these two among the 5 000 of rng_seed = 5.
EMPTY_CLUSTER = {                  # name: (keys, counts, K, seed, the iteration that leaves a cluster empty, the cluster, n of the final iteration)
    "refilled": ([259, 65794, 131331, 197638, 262402, 262404, 263940, 327681, 328199, 328708, 329223, 393732, 459011, 459267, 459523],
                 [1000000, 533, 662, 293, 794, 27, 144, 614, 41, 849, 492, 537, 558, 478, 384], 6, 199306513, 2, 3, [1001195, 558, 1435, 849, 970, 1399]),
    "stays_empty": ([74775, 263429, 329992, 335130, 396293, 402707, 466965, 534033, 598561, 661021, 727562, 730663, 794150, 1052444, 1119490, 1180694, 1311775, 1319719,
                     1446935, 1643789, 1706274, 1707553, 1712394, 1772563, 1906437, 1974289, 2429702],
                    [271, 552, 876, 61, 79, 120, 778, 98, 699, 386, 769, 944, 768, 695, 774, 374, 299, 575, 389, 548, 265, 827, 302, 129, 199, 638, 276], 6, 481771716, 2, 5,
                    [2871, 2986, 3364, 1507, 1963, 0]),
}
EMPTY_MAX_ITER = [1, 2, 3, 300]


# ---- 4. the table kernels
EDGE_KEYS = [0, 15, 16, 4095, 4096, 65535, 65536, (1 << 24) - 4097, (1 << 24) - 4096, (1 << 24) - 1]        # the ends of a thread's 16 bins, of a block's 4096, of the table
EDGE_COUNTS = [11 + 3 * i for i in range(len(EDGE_KEYS))]


def edge_image():
    return weighted_image(EDGE_KEYS, EDGE_COUNTS)


def is_white(keys, thr=240):
    k = np.asarray(keys, np.int64)
    return ((k >> 16) >= thr) & (((k >> 8) & 255) >= thr) & ((k & 255) >= thr)


@functools.lru_cache(maxsize=None)
def every_colour_image():
    """4096 x 4096: each of the 2^24 colours once, shuffled"""
    return key_image(np.random.default_rng(24).permutation(1 << 24).astype(np.uint32), (4096, 4096))


@functools.lru_cache(maxsize=None)
def every_colour_buckets():
    """hue bucket of every key 0 .. 2^24 - 1 (int8)"""
    return np.concatenate([D.hue_buckets_np(np.arange(r << 16, (r + 16) << 16, dtype=np.uint32)).astype(np.int8) for r in range(0, 256, 16)])


def filter_image(nonwhite):
    """16 x 16, `nonwhite` pixels that pass the default filter (one channel 239), the rest (240, 250, 255)"""
    img = np.empty((16, 16, 3), np.uint8); img[:] = (240, 250, 255)
    flat = img.reshape(-1, 3)
    at = np.random.default_rng(16).permutation(256)[:nonwhite]
    flat[at[0::2]] = (255, 239, 255); flat[at[1::2]] = (12, 240, 255)
    return img


THRESHOLD_COLOURS = [(0, 0, 0), (0, 255, 255), (255, 0, 255), (1, 1, 1), (1, 255, 255), (254, 254, 254), (255, 255, 254), (255, 254, 255), (255, 255, 255)]
THRESHOLDS = {                     # white_threshold: the colours of THRESHOLD_COLOURS with a channel below it
    0: [],
    1: [(0, 0, 0), (0, 255, 255), (255, 0, 255)],
    255: THRESHOLD_COLOURS[:-1],
    256: THRESHOLD_COLOURS,
}


def threshold_image():
    return weighted_image([r << 16 | g << 8 | b for r, g, b in THRESHOLD_COLOURS], [3 + i for i in range(len(THRESHOLD_COLOURS))])


def all_white_image():
    return np.full((64, 80, 3), 255, np.uint8)


def one_colour_tail():
    """1001 x 1003 = 1 004 003 pixels = 4 * 251 000 + 3: every wave merges one key, and the last group of four holds three pixels"""
    img = np.empty((1001, 1003, 3), np.uint8); img[:] = (12, 200, 77)
    return img


def two_colour_rows():
    """rows alternate between two colours, 67 pixels a row: a wave's 256 pixels hold both and nothing else (but at the ends), so the two leader rounds of
    an_bin_add take everything; 129 * 67 = 8643 = 4 * 2160 + 3"""
    img = np.empty((129, 67, 3), np.uint8); img[0::2] = (200, 10, 30); img[1::2] = (10, 200, 31)
    return img


def three_colour_rows():
    """the same with three colours: lanes holding the third key of a wave fall through to the single add"""
    img = np.empty((129, 67, 3), np.uint8); img[0::3] = (200, 10, 30); img[1::3] = (10, 200, 31); img[2::3] = (90, 90, 250)
    return img


def keys_per_wave_slot(img):
    """k_an_hist hands a wave 64 groups of four consecutive pixels and calls an_bin_add once per slot j: lane l holds pixel 4 * (64 w + l) + j.  -> the number
    of distinct keys per (wave, slot) over the whole image, as a sorted list of the numbers that occur"""
    px = np.asarray(img, np.uint32).reshape(-1, 3)
    key = px[:, 0] << 16 | px[:, 1] << 8 | px[:, 2]
    n = len(key)
    pad = np.full((-n) % 256, -1, np.int64)
    k = np.concatenate([key.astype(np.int64), pad]).reshape(-1, 64, 4)
    out = set()
    for w in k:
        for j in range(4):
            out.add(len(set(w[:, j].tolist()) - {-1}))
    return sorted(out)
