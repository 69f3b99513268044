"""Where the time of analyze_colors goes (orip/analyze.py, csrc/analyze.hip), on seeded synthetic images of --size x --size pixels:
  synth    : orip.synth.synth_image, 8 flat classes with +-3 noise (a few thousand colours: the flat-artwork end, millions of pixels per bin neighbourhood)
  photo    : smooth colour gradients with noise (hundreds of thousands of colours)
  noise    : uniform random bytes (nearly every pixel its own colour: the upper end of the table)
per image: table (whole call, k_an_hist / k_an_count / k_an_emit), hue (call, k_an_hue), k-means with the tool's defaults K = 8, n_init = 10, max_iter = 300
(call, seeding, Lloyd, iterations), the host steps (exact best init, palette matching + recommendation), and the upload.
--reference also times what the reference does instead, where it can run: sklearn KMeans(8, random_state=42, n_init=10) on a 50 000-pixel sample (:70-77)
and a restatement of its per-pixel Python hue loop (:134-167) on the same sample (its HSV comes from cv2, which is not installed: the double's is used).
usage: python tools/time_analyze.py [--size 4096] [--images synth,photo,noise] [--reps 3] [--reference] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omnirevolve-image-processor_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def make_image(kind, n):
    """BGR uint8 [n, n, 3]"""
    if kind == "synth":
        from orip.synth import synth_image
        return synth_image(n, n, 8)
    rng = np.random.default_rng(7)
    if kind == "noise":
        return rng.integers(0, 256, (n, n, 3), dtype=np.uint8)
    y, x = np.mgrid[0:n, 0:n].astype(np.float32) / n
    img = np.stack([255 * x, 255 * y, 128 + 127 * np.sin(6.0 * (x + y))], 2) + rng.normal(0, 4, (n, n, 3)).astype(np.float32)
    return np.clip(img, 0, 255).astype(np.uint8)


def med(f, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = f(); t.append(time.perf_counter() - t0)
    return float(np.median(t)), r


def kernels(dev, f, names):
    dev.prof_reset(); dev.prof_enable(True); f(); dev.prof_enable(False)
    return {k: dev.prof_get(k)[0] for k in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", default="synth,photo,noise")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orip.device import Device
    from orip import analyze as AN
    res = {"size": a.size, "images": {}}
    dev = Device(0)
    try:
        dev.set_image(make_image("synth", 64)); dev.colors_table(); dev.colors_hue(); dev.colors_kmeans(2, n_init=1, max_iter=2)      # code objects, first buffers
        palette = AN.Palette(None, dev.lab_of_rgb); palette.labs()
        for kind in [k for k in a.images.split(",") if k]:
            bgr = make_image(kind, a.size)
            r = {}
            r["upload_s"], _ = med(lambda: dev.set_image(bgr), a.reps)
            r["table_s"], (_, _, kept, used_all) = med(lambda: dev.colors_table(fetch=False), a.reps)
            r["table_kernels_ms"] = kernels(dev, lambda: dev.colors_table(fetch=False), ("k_an_hist", "k_an_count", "k_an_emit"))
            r["kept_pixels"] = kept; r["colours"] = dev._colors_D
            r["hue_s"], hue = med(dev.colors_hue, a.reps)
            r["hue_kernels_ms"] = kernels(dev, dev.colors_hue, ("k_an_hue",))
            r["kmeans_s"], (cen, n, sums, it) = med(lambda: dev.colors_kmeans(8), a.reps)
            r["kmeans_parts_ms"] = kernels(dev, lambda: dev.colors_kmeans(8), ("an_seed", "an_lloyd"))
            r["kmeans_iterations"] = it.tolist()
            r["best_init_s"], b = med(lambda: AN.best_init(n, sums), a.reps)
            an = AN.ColorAnalyzer(palette)

            def host():
                an.set_clusters(cen[b], n[b]); an.set_hue_counts(hue); return an.recommend_colors(4)
            r["host_recommend_s"], rec = med(host, a.reps)
            r["recommended"] = [x[0] for x in rec]
            if a.reference:
                rgb = bgr[:, :, ::-1].reshape(-1, 3)
                keep = rgb[np.any(rgb < 240, axis=1)]
                sample = keep[np.random.default_rng(0).choice(len(keep), 50000, replace=False)] if len(keep) > 50000 else keep
                try:
                    from sklearn.cluster import KMeans
                    t0 = time.perf_counter(); KMeans(n_clusters=8, random_state=42, n_init=10).fit_predict(sample); r["reference_sklearn_50000_s"] = time.perf_counter() - t0
                except ImportError:
                    r["reference_sklearn_50000_s"] = None
                import analyze_double as D
                t0 = time.perf_counter()
                cats = dict.fromkeys(D.HUE_KEYS, 0)
                for p in sample.tolist():
                    cats[D.hue_bucket(*p)] += 1
                r["reference_hue_loop_50000_s"] = time.perf_counter() - t0
            res["images"][kind] = r
            print(kind, json.dumps(r), flush=True)
    finally:
        dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
