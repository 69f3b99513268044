#!/usr/bin/env python3
"""tests/golden/make_golden_analyze.py -- golden vectors for analyze_colors: what scikit-learn's KMeans, the reference's clusterer
(analyze_colors.py:76), finds on small images whose optimum is unambiguous.

Needs scikit-learn (1.7.2 when the fixture was made); the tests only read the .npz.  The reference's script itself does not start (it imports a
`color_palette` module that does not exist, and cv2), so the statements of :60-102 that matter are restated here around the same sklearn call.
  * img_<c>        : RGB uint8 images, Gaussian colour blobs on a white background, at most 50 000 kept pixels (the reference's path at :70-72 then draws
                     no random subsample, so sklearn sees every kept pixel, as the device does)
  * K_<c>_<K>      : per image and cluster count: inertia_[20] of KMeans(K, random_state=s, n_init=10) for s = 0..19; rgb_ / pct_: the cluster list of
                     :79-102 from random_state=42 (centres truncated with astype(int), percentages, ordered by np.argsort(-sizes))
  * cases          : "<image>:<K>" of the asserted cases -- sklearn's own max / min inertia over the 20 seeds differs by less than 1e-6 relative, which is
                     checked here and is the condition under which "reaches the optimum" is a statement about the data and not about a random stream
  * info_cases     : over-split cases (K above the number of blobs), recorded for information: sklearn itself spreads by percents there; nothing asserts on them
Usage: python tests/golden/make_golden_analyze.py
"""
from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# name, (H, W) of the coloured area inside a white frame, blob means, sigma, seed
IMAGES = [
    ("a", (144, 192), [(200, 40, 40), (40, 160, 60), (40, 60, 190), (230, 200, 50), (120, 60, 150), (60, 60, 60)], 14.0, 11),
    ("b", (120, 160), [(220, 120, 30), (30, 140, 170), (90, 40, 30), (150, 200, 90)], 10.0, 12),
    ("c", (100, 200), [(25, 25, 25), (200, 30, 90), (70, 110, 220), (240, 170, 150), (20, 120, 60)], 8.0, 13),
]
ASSERTED = {"a": [4, 6], "b": [2, 4], "c": [3, 5]}
INFO = {"a": [8, 12]}


def blob_image(shape, means, sigma, seed):
    """blobs as vertical bands of equal width inside a 16-pixel white frame"""
    rng = np.random.default_rng(seed)
    h, w = shape
    img = np.full((h + 32, w + 32, 3), 255, np.uint8)
    band = np.minimum(np.arange(w) * len(means) // w, len(means) - 1)
    body = np.asarray(means, np.float64)[band][None, :, :] + rng.normal(0.0, sigma, (h, w, 3))
    img[16:16 + h, 16:16 + w] = np.clip(np.rint(body), 0, 255).astype(np.uint8)
    return img


def kept(img):
    pixels = img.reshape(-1, 3)
    return pixels[np.any(pixels < 240, axis=1)]              # :60-61


def main():
    from sklearn.cluster import KMeans
    import sklearn
    g = {"sklearn_version": np.array(sklearn.__version__)}
    cases, info = [], []
    for name, shape, means, sigma, seed in IMAGES:
        img = blob_image(shape, means, sigma, seed)
        px = kept(img)
        assert 100 <= len(px) <= 50000, len(px)
        g[f"img_{name}"] = img
        for K in ASSERTED.get(name, []) + INFO.get(name, []):
            inert = np.array([KMeans(n_clusters=K, random_state=s, n_init=10).fit(px).inertia_ for s in range(20)], np.float64)
            spread = float(inert.max() / inert.min() - 1.0)
            km = KMeans(n_clusters=K, random_state=42, n_init=10)                           # :76
            labels = km.fit_predict(px)
            centers = km.cluster_centers_.astype(int)                                       # :80
            sizes = np.bincount(labels)                                                     # :83
            order = np.argsort(-sizes)                                                      # :87
            g[f"K_{name}_{K}_inertia"] = inert
            g[f"K_{name}_{K}_rgb"] = centers[order].astype(np.int64)
            g[f"K_{name}_{K}_pct"] = (sizes / len(labels) * 100)[order]
            asserted = K in ASSERTED.get(name, [])
            print(f"image {name}: {len(px)} kept pixels, K={K}: sklearn spread over 20 seeds {spread:.3e} ({'asserted' if asserted else 'information only'})")
            if asserted:
                assert spread < 1e-6, f"image {name}, K={K}: the optimum is ambiguous for sklearn itself (spread {spread:.3e}); not a usable case"
                cases.append(f"{name}:{K}")
            else:
                info.append(f"{name}:{K}")
    g["cases"] = np.array(cases); g["info_cases"] = np.array(info)
    out = os.path.join(HERE, "golden_analyze.npz")
    np.savez_compressed(out, **g)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
