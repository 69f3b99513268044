"""numpy / Python restatement of the device side of analyze_colors (include/orip.h: orip_colors_table, orip_colors_hue, orip_colors_kmeans), written from
the definitions and not from the kernels: the filter, the colour table, OpenCV's 8-bit RGB2HSV and the hue buckets, the k-means++ seeding with Python
integers, Lloyd in float64 with the same expression order, and the exact choice of the best init.  hue_counts_np and first_draw_seeds are vectorised forms
of hue_counts and of the first draw, for tables and seed searches of millions.  Test infrastructure; nothing here runs on a GPU."""
from fractions import Fraction

import numpy as np

HUE_KEYS = ["red", "orange", "yellow", "green", "cyan", "blue", "purple", "pink", "brown", "gray", "black"]
M64 = (1 << 64) - 1


def kept_pixels(rgb, ignore_white=True, white_threshold=240, min_kept=100):
    """analyze_colors.py:58-67 -> (pixels [n,3] uint8, used_all)"""
    px = np.asarray(rgb, np.uint8).reshape(-1, 3)
    if not ignore_white:
        return px, False
    kept = px[np.any(px.astype(np.int64) < white_threshold, axis=1)]
    if len(kept) < min_kept:
        return px, True
    return kept, False


def color_table(rgb, ignore_white=True, white_threshold=240, min_kept=100):
    """(keys uint32 [D] ascending, counts int64 [D], kept pixels, used_all)"""
    px, used_all = kept_pixels(rgb, ignore_white, white_threshold, min_kept)
    key = (px[:, 0].astype(np.uint32) << 16) | (px[:, 1].astype(np.uint32) << 8) | px[:, 2].astype(np.uint32)
    keys, counts = np.unique(key, return_counts=True)
    return keys.astype(np.uint32), counts.astype(np.int64), int(len(px)), used_all


def _rnd_div(a, b):
    """round(a / b) for positive integers (no ties occur for the two tables)"""
    assert (2 * a) % b != 0 or ((2 * a) // b) % 2 == 0
    return (2 * a + b) // (2 * b)


SDIV = [0] + [_rnd_div(255 << 12, i) for i in range(1, 256)]
HDIV = [0] + [_rnd_div(180 << 12, 6 * i) for i in range(1, 256)]


def hsv8(r, g, b):
    """OpenCV COLOR_RGB2HSV on uint8 (h 0..179), integer path, as recalled"""
    r, g, b = int(r), int(g), int(b)
    v = max(r, g, b)
    diff = v - min(r, g, b)
    s = (diff * SDIV[v] + (1 << 11)) >> 12
    if v == r:
        h = g - b
    elif v == g:
        h = b - r + 2 * diff
    else:
        h = r - g + 4 * diff
    h = (h * HDIV[diff] + (1 << 11)) >> 12
    if h < 0:
        h += 180
    return h, s, v


def hue_bucket(r, g, b):
    """analyze_colors.py:134-167 for one colour -> bucket name"""
    h, s, v = hsv8(r, g, b)
    if v < 50:
        return "black"
    if s < 30:
        return "gray"
    h_full = h * 2
    if h_full < 15 or h_full >= 345:
        return "red"
    if h_full < 25:
        return "brown" if (s > 150 and v < 150) else "orange"
    if h_full < 45:
        return "orange"
    if h_full < 75:
        return "yellow"
    if h_full < 150:
        return "green"
    if h_full < 200:
        return "cyan"
    if h_full < 270:
        return "blue"
    if h_full < 330:
        return "pink" if s < 100 else "purple"
    return "pink"


def hue_counts(keys, counts):
    out = dict.fromkeys(HUE_KEYS, 0)
    for k, c in zip(keys.tolist(), counts.tolist()):
        out[hue_bucket(k >> 16, (k >> 8) & 255, k & 255)] += c
    return np.array([out[k] for k in HUE_KEYS], np.int64)


SDIV_NP, HDIV_NP = np.array(SDIV, np.int64), np.array(HDIV, np.int64)


def hue_buckets_np(keys):
    """hue_bucket for an array of keys at once -> index into HUE_KEYS per key.  int64 throughout: >> floors like Python's, h may be negative before the + 180.
    tests/test_analyze_cases_host.py pins it to the scalar hue_bucket."""
    k = np.asarray(keys).astype(np.int64)
    r, g, b = k >> 16, (k >> 8) & 255, k & 255
    v = np.maximum(r, np.maximum(g, b))
    diff = v - np.minimum(r, np.minimum(g, b))
    s = (diff * SDIV_NP[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV_NP[diff] + (1 << 11)) >> 12
    hf = 2 * np.where(h < 0, h + 180, h)
    ix = {n: i for i, n in enumerate(HUE_KEYS)}
    conds = [v < 50, s < 30, (hf < 15) | (hf >= 345), hf < 25, hf < 45, hf < 75, hf < 150, hf < 200, hf < 270, hf < 330]
    picks = [ix["black"], ix["gray"], ix["red"], np.where((s > 150) & (v < 150), ix["brown"], ix["orange"]), ix["orange"], ix["yellow"], ix["green"], ix["cyan"],
             ix["blue"], np.where(s < 100, ix["pink"], ix["purple"])]
    return np.select(conds, picks, ix["pink"]).astype(np.int64)


def hue_counts_np(keys, counts):
    """hue_counts without the Python loop per colour"""
    out = np.zeros(len(HUE_KEYS), np.int64)
    np.add.at(out, hue_buckets_np(keys), np.asarray(counts, np.int64))
    return out


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def splitmix64_np(x):
    """splitmix64 of a uint64 array (uint64 arithmetic wraps modulo 2^64)"""
    x = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def first_draw_seeds(total, wanted, limit=1 << 23):
    """the smallest seed below `limit` whose first draw of init 0, splitmix64(seed) % total, equals w, for every w of `wanted` -> {w: seed}.  With every
    count 1, total = D and the draw is the table index of the first centre."""
    t = splitmix64_np(np.arange(limit, dtype=np.uint64)) % np.uint64(total)
    out = {}
    for w in wanted:
        hit = np.flatnonzero(t == np.uint64(w))
        if len(hit):
            out[int(w)] = int(hit[0])
    return out


def seed_indices(keys, counts, K, seed, init):
    """k-means++ with one candidate per step, exact integers -> table indices of the K seeds"""
    rgb = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], 1).astype(np.int64)
    cnt = counts.astype(np.int64)
    mind2 = None
    chosen = []
    for step in range(K):
        w = cnt if step == 0 else cnt * mind2                     # <= 195075 * 2^31: int64 holds every weight and every prefix sum
        pre = np.cumsum(w)
        total = int(pre[-1])
        t = splitmix64((seed ^ ((init << 32) + step)) & M64) % total
        i = int(np.searchsorted(pre, t, side="right"))           # the first inclusive prefix sum > t
        chosen.append(i)
        d2 = ((rgb - rgb[i]) ** 2).sum(1)
        mind2 = d2 if mind2 is None else np.minimum(mind2, d2)
    return chosen


def lloyd(keys, counts, centres, max_iter):
    """-> (centres float64 [K,3], n int64 [K], sums int64 [K,3], iterations)"""
    r = (keys >> 16).astype(np.float64); g = ((keys >> 8) & 255).astype(np.float64); b = (keys & 255).astype(np.float64)
    ch = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], 1).astype(np.int64)
    cnt = counts.astype(np.int64)
    c = np.array(centres, np.float64)
    K = len(c)
    labels = np.full(len(keys), -1, np.int64)
    for it in range(1, max_iter + 1):
        d = np.stack([((r - c[k, 0]) ** 2 + (g - c[k, 1]) ** 2) + (b - c[k, 2]) ** 2 for k in range(K)], 1)
        new = np.argmin(d, axis=1)                               # the first minimum: ties to the lowest index
        changed = int((new != labels).sum())
        labels = new
        n = np.zeros(K, np.int64); sums = np.zeros((K, 3), np.int64)
        np.add.at(n, labels, cnt)
        np.add.at(sums, labels, cnt[:, None] * ch)
        for k in range(K):
            if n[k] > 0:
                c[k] = sums[k].astype(np.float64) / np.float64(n[k])
        if changed == 0:
            break
    return c, n, sums, it


def kmeans(keys, counts, K, n_init=10, max_iter=300, seed=42):
    """every init: (centres [n_init,K,3], n [n_init,K], sums [n_init,K,3], iterations [n_init])"""
    if len(keys) < K:
        raise ValueError("fewer distinct colours than clusters")
    rgb = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], 1).astype(np.float64)
    out = [lloyd(keys, counts, rgb[seed_indices(keys, counts, K, seed, i)], max_iter) for i in range(n_init)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]), np.array([o[3] for o in out], np.int32))


def inertia_exact(keys, counts, n, sums):
    s2 = sum(int(c) * ((int(k) >> 16) ** 2 + ((int(k) >> 8) & 255) ** 2 + (int(k) & 255) ** 2) for k, c in zip(keys, counts))
    return Fraction(s2) - sum((Fraction(sum(int(v) ** 2 for v in sums[k]), int(n[k])) for k in range(len(n)) if n[k] > 0), Fraction(0))


def best_init(keys, counts, n, sums):
    """smallest exact inertia, ties to the lowest index"""
    vals = [inertia_exact(keys, counts, n[i], sums[i]) for i in range(len(n))]
    return min(range(len(vals)), key=lambda i: (vals[i], i))


def pixel_inertia(pixels, centres):
    """float64 inertia of `centres` over pixels [n,3]: every pixel to its nearest centre"""
    p = np.asarray(pixels, np.float64); c = np.asarray(centres, np.float64)
    d = ((p[:, None, :] - c[None]) ** 2).sum(-1)
    return float(d.min(1).sum())


# A hand-checked colour list: (colour, (h, s, v) of OpenCV's 8-bit HSV, bucket), one colour on each side of every threshold.
# h = 30 * ((mid - min) / diff + 2 * sector) rounded, s = 255 * diff / v rounded; the colours sit >= 0.06 away from a rounding boundary.
HUE_LIST = [
    ((49, 10, 10), (0, 203, 49), "black"), ((50, 10, 10), (0, 204, 50), "red"),                   # v < 50
    ((200, 177, 177), (0, 29, 200), "gray"), ((200, 176, 176), (0, 31, 200), "red"),              # s < 30
    ((200, 77, 40), (7, 204, 200), "red"), ((200, 82, 40), (8, 204, 200), "orange"),              # h_full < 15
    ((200, 103, 40), (12, 204, 200), "orange"), ((200, 109, 40), (13, 204, 200), "orange"),       # h_full < 25 (s > 150 but v >= 150: not brown)
    ((140, 84, 57), (10, 151, 140), "brown"), ((140, 85, 58), (10, 149, 140), "orange"),          # s > 150
    ((149, 80, 40), (11, 187, 149), "brown"), ((150, 80, 40), (11, 187, 150), "orange"),          # v < 150
    ((200, 157, 40), (22, 204, 200), "orange"), ((200, 162, 40), (23, 204, 200), "yellow"),       # h_full < 45
    ((162, 200, 40), (37, 204, 200), "yellow"), ((157, 200, 40), (38, 204, 200), "green"),        # h_full < 75
    ((40, 200, 114), (74, 204, 200), "green"), ((40, 200, 119), (75, 204, 200), "cyan"),          # h_full < 150
    ((40, 151, 200), (99, 204, 200), "cyan"), ((40, 146, 200), (100, 204, 200), "blue"),          # h_full < 200
    ((114, 40, 200), (134, 204, 200), "blue"), ((119, 40, 200), (135, 204, 200), "purple"),       # h_full < 270
    ((230, 141, 215), (155, 99, 230), "pink"), ((230, 139, 215), (155, 101, 230), "purple"),      # s < 100 inside 270..330
    ((200, 40, 125), (164, 204, 200), "purple"), ((200, 40, 119), (165, 204, 200), "pink"),       # h_full < 330
    ((200, 40, 82), (172, 204, 200), "pink"), ((200, 40, 77), (173, 204, 200), "red"),            # h_full >= 345
    ((0, 0, 0), (0, 0, 0), "black"), ((255, 255, 255), (0, 0, 255), "gray"),
]


class DoubleDevice:
    """the Device methods ColorAnalyzer.analyze uses, served by the numpy double"""

    def __init__(self, rgb):
        self.rgb = np.asarray(rgb, np.uint8); self.H, self.W = self.rgb.shape[:2]

    def colors_table(self, ignore_white=True, white_threshold=240, min_kept=100, fetch=True):
        self.keys, self.counts, kept, used_all = color_table(self.rgb, ignore_white, white_threshold, min_kept)
        return (self.keys, self.counts, kept, used_all) if fetch else (None, None, kept, used_all)

    def colors_kmeans(self, K, n_init=10, max_iter=300, seed=42):
        return kmeans(self.keys, self.counts, K, n_init, max_iter, seed)

    def colors_hue(self):
        return hue_counts(self.keys, self.counts)


def lab_cpu(rgb):
    from oracle import oracle as O
    return O.bgr2lab(np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(-1, 3)[:, ::-1]))
