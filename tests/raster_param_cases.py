"""Inputs and parameter lists of the raster sweeps: stage 02 (k-means fit, assignment, label masks) and stage 03 (edges) away from their default
arguments and at small shapes.  tests/test_oracle_raster_params.py (CPU) asserts on the oracle alone that every input does what it was chosen
for; tests/test_gpu_raster_params.py (GPU) compares the device with the oracle over the same lists.  Plain data and numpy (scipy.ndimage for
the smoothing): nothing here touches the oracle or the device."""
import numpy as np
from scipy.ndimage import gaussian_filter

# the odd shapes of tests/test_gpu_raster.py (the CPU test asserts that the two lists are the same)
ODD_SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (3, 63), (5, 64), (5, 65), (17, 127), (33, 129), (64, 191), (9, 257)]


# ---------------------------------------------------------------- k-means
KM_DEFAULT = (3, 40, 0.5)            # attempts, max_iter, eps of every other fit of the suite


def noise_bgr(seed, shape):
    """uniform-noise BGR image, drawn as uint8 (the stream of test_kmeans_random_pixels_matches_oracle)"""
    return np.random.default_rng(seed).integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)


ATTEMPT_SHAPE = (60, 70)
# (seed, K, attempts): the LAST attempt (index attempts - 1) is the one that wins, i.e. a fit with one attempt fewer ends less compact.  Under the
# device's schedule (four groups, group g runs the attempts g, g + 4, g + 8) that attempt is:
ATTEMPT_CASES = [
    (6, 6, 1),       # group 0, first attempt (one group in all)
    (6, 6, 2),       # group 1 of two
    (8, 6, 4),       # group 3, first attempt: the host's choice among four groups
    (6, 6, 5),       # group 0, SECOND attempt: re-initialisation and the in-group choice
    (0, 3, 7),       # group 2, second attempt
    (0, 3, 8),       # group 3, second attempt
    (8, 6, 9),       # group 0, THIRD attempt
]
# (seed, K, attempts): an EARLIER attempt wins, the later ones of its group and of the other groups must not replace it
ATTEMPT_KEEP_CASES = [(0, 3, 5), (6, 6, 6), (8, 6, 8)]

SWEEP_IMAGE = dict(seed=9, shape=(90, 110), K=5)        # the image of test_kmeans_random_pixels_matches_oracle
MAX_ITERS = [0, 1, 2, 3, 5, 10, 100, 1000]
EPSES = [-1.0, 0.0, 0.01, 2.0, 5.0, 50.0, 1e9]
MAX_ITERS_RGB = [1, 5, 1000]
EPSES_RGB = [-1.0, 2.0, 1e9]
# groups of values that give ONE result on the oracle (clamps of max_iter to 2 .. 100, of eps below 0; a large eps stops after the first update)
MAX_ITER_GROUPS = [[0, 1, 2], [3], [5], [10], [100, 1000]]
EPS_GROUPS = [[-1.0, 0.0, 0.01], [2.0], [5.0], [50.0, 1e9]]


def km_combos(n=6, seed=202):
    rng = np.random.default_rng(seed)
    att, mi, ep = [1, 2, 3, 4, 5, 6, 7, 9], [0, 1, 2, 3, 4, 7, 10, 25, 100, 1000], [-1.0, 0.0, 0.01, 0.5, 1.0, 2.0, 5.0, 50.0]
    return [(att[int(rng.integers(len(att)))], mi[int(rng.integers(len(mi)))], ep[int(rng.integers(len(ep)))]) for _ in range(n)]


# (K, N): as many samples as centres, one more, and sample counts around one wave
TINY_CASES = [(1, 1), (2, 2), (16, 16), (1, 2), (2, 3), (16, 17), (4, 63), (4, 64), (4, 65)]


def tiny_indices(K, N, npx=ATTEMPT_SHAPE[0] * ATTEMPT_SHAPE[1]):
    return np.random.default_rng(1000 * K + N).choice(npx, N, replace=False).astype(np.int64)


# The device gives thread g of a group's 16 384 the samples [g * chunk, (g + 1) * chunk) below N, chunk = ceil(N / 16 384).  Sample counts at which the
# chunk length changes: lengths 1, 1, 2, 2, 3, 3, 4; at 16 385 the upper half of the workgroups owns nothing and the last thread that owns anything owns
# one sample.  The samples are the first N pixels of the image, K and the other arguments below.
CHUNK_IMAGE = dict(seed=21, shape=(193, 255), K=5)
CHUNK_NS = [16383, 16384, 16385, 32768, 32769, 49152, 49153]
CHUNK_N_RGB = 16385              # this one through the RGB fit as well


def two_colour_bgr(shape=(40, 50)):
    """two colours in random positions: every attempt with K = 2 ends exactly as compact as every other, and which colour is centre 0 follows from the
    attempt's first draw -- only the choice among EQUAL attempts decides the centres' order"""
    rng = np.random.default_rng(84)
    pick = rng.integers(0, 2, shape)
    return np.where(pick[:, :, None] == 0, np.array([30, 60, 200], np.uint8), np.array([220, 180, 40], np.uint8)).astype(np.uint8)


def rng_first_indices(N, K, attempts):
    """the first centre index of every attempt: cv::RNG (multiply with carry, 4164903690, state 2^32 - 1), one draw for the index and 6 (K - 1) for the
    three trials of each further centre"""
    st = 0xffffffff
    out = []
    for _ in range(attempts):
        for q in range(1 + 6 * (K - 1)):
            st = ((st & 0xffffffff) * 4164903690 + (st >> 32)) & 0xffffffffffffffff
            if q == 0:
                out.append((st & 0xffffffff) % N)
    return out


def bright_bgr(side):
    """bright image whose channel sums pass 2^24 within one cluster: the centre update adds float32 in sample order there"""
    return np.clip(np.random.default_rng(3).normal(225, 18, (side, side, 3)), 0, 255).astype(np.uint8)


F32_SIDE_K1 = 300
F32_SIDE_K2 = 380            # the CPU test asserts that this is the first multiple of 10 at which a cluster's sum reaches 2^24 with K = 2
F32_K2_ARGS = (1, 6, 0.0)    # attempts, max_iter, eps


# ---------------------------------------------------------------- stage 02: assignment and masks
ITER_PAIRS02 = [(0, 0), (0, 1), (1, 0), (2, 1), (1, 3), (3, 3)]
SHAPES02 = ODD_SHAPES + [(64, 64), (8, 128), (33, 192), (5, 256)]       # the last four: rows of whole 64-pixel words
KS02 = [2, 3, 16]
TIE_SHAPE = (33, 129)


def speckle_bgr(shape, seed=None):
    """lightly smoothed noise: a speckled label map on which every morphology pass changes something"""
    H, W = shape
    rng = np.random.default_rng(H * 131 + W if seed is None else seed)
    v = gaussian_filter(rng.random((H, W, 3)), (0.8, 0.8, 0), mode="nearest")
    lo, hi = v.min(), v.max()
    return ((v - lo) / (hi - lo) * 255 if hi > lo else v * 255).astype(np.uint8)


def centres_from(lab, K, seed=5):
    """K explicit centres: the Lab of K seeded pixels of the image, moved by a fraction (float32)"""
    flat = np.asarray(lab).reshape(-1, 3).astype(np.float64)
    rng = np.random.default_rng(seed * 100 + K)
    pos = rng.integers(0, len(flat), K)
    return (flat[pos] + rng.uniform(-6.0, 6.0, (K, 3))).astype(np.float32)


# ---------------------------------------------------------------- stage 03
SHAPE03 = (97, 131)
DEFAULTS03 = dict(edge_morph_kernel=3, edge_morph_open_iters=1, edge_morph_close_iters=1, edge_kernel_size=3, edge_low_threshold=50, edge_high_threshold=150)


def binary_mask(shape, seed=None, t=0.0):
    H, W = shape
    rng = np.random.default_rng(H * 77 + W if seed is None else seed)
    return (gaussian_filter(rng.standard_normal((H, W)), 1.5, mode="nearest") > t).astype(np.uint8) * 255


def grey_mask(shape, seed=None):
    H, W = shape
    rng = np.random.default_rng(H * 91 + W + 1 if seed is None else seed)
    m = gaussian_filter(rng.random((H, W)) * 255, 1.0, mode="nearest")
    lo, hi = m.min(), m.max()
    return ((m - lo) / (hi - lo) * 255).astype(np.uint8) if hi > lo else np.full((H, W), 128, np.uint8)


MASK_KINDS = dict(binary=binary_mask, grey=grey_mask)

MORPH_KERNELS03 = [1, 5, 7]
ITERS03 = [dict(edge_morph_open_iters=0, edge_morph_close_iters=0), dict(edge_morph_open_iters=0, edge_morph_close_iters=1),
           dict(edge_morph_open_iters=1, edge_morph_close_iters=0), dict(edge_morph_open_iters=2, edge_morph_close_iters=1),
           dict(edge_morph_open_iters=1, edge_morph_close_iters=3), dict(edge_morph_open_iters=3, edge_morph_close_iters=2, edge_morph_kernel=5)]
GAUSS_KERNELS03 = [1, 2, 4, 5, 6, 7]
GAUSS_SAME03 = [(1, 3), (2, 3), (4, 5), (6, 7)]                  # ensure_odd (03:9-11): these pairs are one kernel
THRESHOLDS03 = [(0, 150), (-5, 150), (150, 150), (151, 150), (400, 100), (100, 400), (50, 50), (50, 600), (50, 2039), (50, 2040), (0, 0)]
THRESHOLD_TWINS03 = ((400, 100), (100, 400))

ONE_AT_A_TIME03 = ([dict(edge_morph_kernel=k) for k in MORPH_KERNELS03] + ITERS03 + [dict(edge_kernel_size=k) for k in GAUSS_KERNELS03]
                   + [dict(edge_low_threshold=lo, edge_high_threshold=hi) for lo, hi in THRESHOLDS03])


def combos03(n=8, seed=303):
    rng = np.random.default_rng(seed)
    R = dict(edge_morph_kernel=[1, 3, 5, 7], edge_morph_open_iters=[0, 1, 2, 3], edge_morph_close_iters=[0, 1, 2, 3], edge_kernel_size=[1, 3, 4, 5, 7],
             edge_low_threshold=[0, 20, 50, 150, 400], edge_high_threshold=[0, 60, 150, 300, 600])
    return [{k: v[int(rng.integers(len(v)))] for k, v in R.items()} for _ in range(n)]


SHAPES03 = ODD_SHAPES + [(7, 7), (7, 8), (8, 7), (8, 8), (8, 64), (7, 128), (64, 64), (16, 192)]     # around the 8-pixel and the 64-column switches
SHAPE_BASE03 = dict(edge_low_threshold=20, edge_high_threshold=60)
SHAPE_SETS03 = dict(
    A=dict(edge_kernel_size=5),
    B=dict(edge_kernel_size=7, edge_morph_kernel=1),
    C=dict(edge_morph_kernel=5, edge_morph_open_iters=0),
    D=dict(edge_morph_kernel=7, edge_morph_open_iters=0, edge_morph_close_iters=2),
    E=dict(edge_kernel_size=7, edge_morph_kernel=7),
    F=dict(edge_morph_open_iters=0, edge_morph_close_iters=0),
    G=dict(edge_kernel_size=5, edge_morph_kernel=5, edge_morph_open_iters=2, edge_morph_close_iters=3),
)
LAYERS_SHAPE03 = (33, 129)
LAYERS_SET03 = "G"
REFUSED_GAUSS03 = [9]
REFUSED_MORPH03 = [2, 8, 9]


def cfg03(*parts):
    d = dict(DEFAULTS03)
    for p in parts:
        d.update(p)
    return d


# ---------------------------------------------------------------- stage 02: ties, all colours
def tie_centres(lab):
    """centre sets on which the order of equal things decides (lab: the Lab of speckle_bgr(TIE_SHAPE))"""
    flat = np.asarray(lab).reshape(-1, 3).astype(np.float32)
    med = np.median(flat, axis=0)
    L, a, b = float(med[0]), float(med[1]), float(med[2])
    return dict(
        equal_L=np.array([[L, a + 9.0, b], [L, a - 9.0, b], [L - 30.0, a, b]], np.float32),          # the stable sort keeps 0 in front of 1
        identical=np.array([[L + 10.0, a, b], [L + 10.0, a, b], [L - 10.0, a, b]], np.float32),      # the second of two equal centres never wins
        equidistant=np.array([[L + 1.0, a, b], [L - 1.0, a, b]], np.float32),                        # every pixel with lightness L is as far from both
        equidistant_swapped=np.array([[L - 1.0, a, b], [L + 1.0, a, b]], np.float32),
    )


def all_colours():
    """every 24-bit colour once: (BGR image 4096 x 4096, the same colours as R, G, B triples)"""
    i = np.arange(1 << 24, dtype=np.uint32)
    bgr = np.stack([i & 255, (i >> 8) & 255, i >> 16], 1).astype(np.uint8)
    return bgr.reshape(4096, 4096, 3), np.ascontiguousarray(bgr[:, ::-1])
