"""Host side of analyze_colors.py (the reference's marker-recommendation tool): the producer of the "recommended_colors" file that
process_colors.py --mode palette reads.  The data-parallel steps run in liborip.so (csrc/analyze.hip: orip_colors_table, orip_colors_hue,
orip_colors_kmeans, orip_lab_of_rgb) on EVERY kept pixel; what stays here is the reference's host logic, line by line, the exact choice of the best
k-means init, and the palette.  Citations: image_processor/analyze_colors.py of the reference.

What is ours, because the reference does not define it:
  * Palette -- the reference imports a `color_palette.CariocaPalette` that it does not contain (:16).  The distance here is the Euclidean distance between
    8-bit Lab triples (stage 02's BGR2LAB), taken as integers without wrap-around: the scale on which the caller's thresholds 50 / 40 / 35 / 30 make sense.
  * the k-means (include/orip.h: orip_colors_kmeans) instead of sklearn's random stream, and the choice of the best init by exact rational inertia.
`analyzed_pixels` and every percentage refer to all kept pixels of the image, not to a random 50 000-pixel sample (:70-72)."""
from __future__ import annotations

import json
from fractions import Fraction
from typing import Callable, Dict, List, Sequence, Tuple

import numpy as np

HUE_KEYS = ["red", "orange", "yellow", "green", "cyan", "blue", "purple", "pink", "brown", "gray", "black"]        # :128-132, the reference's key order

# A generic set of felt-tip marker colours of our own.  NOT the Carioca palette: the reference's data do not exist (its color_palette module is missing),
# and nothing here was measured from real pens.  Bring the colours of your own box with --palette.
DEFAULT_MARKERS: Dict[str, Tuple[int, int, int]] = {
    "black": (20, 20, 20), "dark_gray": (80, 80, 80), "gray": (140, 140, 140), "light_gray": (200, 200, 200),
    "brown": (120, 70, 40), "dark_brown": (80, 45, 25), "ochre": (200, 150, 60), "skin": (240, 200, 170),
    "red": (220, 30, 40), "dark_red": (150, 20, 30), "orange": (245, 130, 30), "yellow": (250, 225, 40),
    "light_green": (140, 200, 70), "green": (40, 150, 70), "dark_green": (20, 90, 50), "turquoise": (30, 170, 170),
    "light_blue": (100, 180, 235), "blue": (30, 90, 200), "dark_blue": (25, 45, 120), "violet": (120, 60, 170),
    "purple": (150, 40, 120), "magenta": (220, 50, 150), "pink": (245, 150, 190), "salmon": (245, 140, 120),
}


class Palette:
    """Stands in for the reference's missing CariocaPalette: `colors` {name: (r, g, b)} in palette order, find_closest, get_color_group, load.
    lab_of_rgb: R, G, B triples [n,3] -> 8-bit Lab [n,3]; Device.lab_of_rgb on the product path (the same Lab as stage 02).  The built-in default is
    DEFAULT_MARKERS, a generic marker set of our own -- it is not the Carioca palette."""

    def __init__(self, colors: Dict[str, Sequence[int]] | None = None, lab_of_rgb: Callable | None = None):
        src = DEFAULT_MARKERS if colors is None else colors
        self.colors: Dict[str, Tuple[int, int, int]] = {str(k): tuple(int(c) for c in v) for k, v in src.items()}
        if not self.colors:
            raise ValueError("empty palette")
        for k, v in self.colors.items():
            if len(v) != 3 or min(v) < 0 or max(v) > 255:
                raise ValueError(f"palette colour {k!r}: {v} is not an 8-bit R, G, B triple")
        self._lab_fn = lab_of_rgb
        self._labs = None

    def _lab(self, rgb) -> np.ndarray:
        if self._lab_fn is None:
            raise RuntimeError("Palette has no lab_of_rgb: pass Device.lab_of_rgb (there is no CPU fallback in the product)")
        a = np.asarray(rgb, np.int64).reshape(-1, 3)
        if a.min() < 0 or a.max() > 255:
            raise ValueError(f"not 8-bit colours: {a.tolist()}")
        return np.asarray(self._lab_fn(a.astype(np.uint8)), np.int64).reshape(-1, 3)

    def labs(self) -> np.ndarray:
        """int64 [n,3]: 8-bit Lab of the palette colours, in palette order"""
        if self._labs is None:
            self._labs = self._lab(list(self.colors.values()))
        return self._labs

    def _distances(self, lab: np.ndarray) -> np.ndarray:
        return np.sqrt(((self.labs() - lab.reshape(1, 3)) ** 2).sum(1).astype(np.float64))

    def find_closest(self, rgb, n: int = 1) -> List[Tuple[str, float]]:
        """the first n of (name, distance), sorted by distance, then by palette order"""
        d = self._distances(self._lab(rgb)[0])
        names = list(self.colors)
        return [(names[i], float(d[i])) for i in np.argsort(d, kind="stable")[:n]]

    def get_color_group(self, name: str, tolerance: float) -> List[str]:
        """the names whose distance to `name` is at most `tolerance`, in palette order, the colour itself included"""
        names = list(self.colors)
        d = self._distances(self.labs()[names.index(name)])
        return [nm for nm, v in zip(names, d) if v <= tolerance]

    @classmethod
    def load(cls, path: str, lab_of_rgb: Callable | None = None) -> "Palette":
        """the "palette" layout ({"palette": [{"name", "rgb"}]}) and the "colors" layout that process_colors.py writes ({"colors": [{"index", "name", "rgb"}]},
        orip.colors.palette_dump); a missing name becomes color_<i>"""
        with open(path, "r", encoding="utf-8") as f:
            data = json.load(f)
        for key in ("palette", "colors"):
            if key in data:
                items = data[key]
                if key == "colors":
                    items = sorted(items, key=lambda it: it.get("index", 1 << 30))
                return cls({str(it.get("name", f"color_{i}")): it["rgb"] for i, it in enumerate(items)}, lab_of_rgb)
        raise ValueError(f"Unsupported palette JSON structure: {path}")


def best_init(n: np.ndarray, sums: np.ndarray) -> int:
    """index of the init with the smallest inertia sum count |x|^2 - sum_k |sum_k|^2 / n_k.  The first term is the same for every init, so the largest
    sum_k |sum_k|^2 / n_k wins; compared as exact rationals (Python integers), ties to the lowest index.  No floating sum decides anything."""
    best, best_v = 0, None
    for i in range(len(n)):
        v = Fraction(0)
        for k in range(n.shape[1]):
            nk = int(n[i, k])
            if nk > 0:
                v += Fraction(sum(int(s) ** 2 for s in sums[i, k]), nk)
        if best_v is None or v > best_v:
            best, best_v = i, v
    return best


class ColorAnalyzer:
    """ColorAnalyzer of the reference (:19-242) on the image resident in a Device."""

    def __init__(self, palette: Palette):
        self.palette = palette
        self.dominant_colors: List[dict] = []
        self.color_histogram = None
        self.recommendations: List[Tuple[str, float]] = []
        self.used_all_pixels = False

    def set_clusters(self, centers_rgb, sizes) -> None:
        """:79-102 -- centres truncated with astype(int), percentages of all clustered pixels, clusters by size descending (stably), each with its closest
        palette colour"""
        cluster_centers = np.asarray(centers_rgb, np.float64).reshape(-1, 3).astype(int)          # :80
        cluster_sizes = np.asarray(sizes, np.int64).reshape(-1)                                   # :83
        cluster_percentages = cluster_sizes / max(int(cluster_sizes.sum()), 1) * 100              # :84
        self.dominant_colors = []
        for idx in np.argsort(-cluster_sizes, kind="stable"):                                     # :87
            color_rgb = tuple(int(v) for v in cluster_centers[idx])
            closest = self.palette.find_closest(color_rgb, n=1)[0]                                # :95
            self.dominant_colors.append({"rgb": color_rgb, "percentage": float(cluster_percentages[idx]), "closest_palette": closest[0], "distance": closest[1]})

    def set_dominant(self, rgbs, percentages) -> None:
        """the same list from recorded (rgb, percentage) pairs, already ordered (a fixture, another clusterer)"""
        self.dominant_colors = []
        for rgb, pct in zip(rgbs, percentages):
            color_rgb = tuple(int(v) for v in rgb)
            closest = self.palette.find_closest(color_rgb, n=1)[0]
            self.dominant_colors.append({"rgb": color_rgb, "percentage": float(pct), "closest_palette": closest[0], "distance": closest[1]})

    def set_hue_counts(self, counts) -> None:
        """:169-173 -- percentages of the bucket counts"""
        c = {k: int(v) for k, v in zip(HUE_KEYS, counts)}
        total = sum(c.values())
        self.color_histogram = {k: v / total * 100 for k, v in c.items()} if total > 0 else c

    def analyze(self, dev, n_clusters: int = 8, ignore_white: bool = True, white_threshold: int = 240, n_init: int = 10, max_iter: int = 300, seed: int = 42) -> Dict:
        """:28-116 on the image set in `dev` (Device.set_image).  Every kept pixel is clustered: there is no subsample."""
        _, _, kept, used_all = dev.colors_table(ignore_white, white_threshold, 100, fetch=False)          # :58-67
        self.used_all_pixels = used_all
        if used_all:
            print("Warning: Image is mostly white, using all pixels")                                     # :65
        print(f"Clustering {kept} pixels into {n_clusters} groups...")                                    # :75
        centers, n, sums, _ = dev.colors_kmeans(n_clusters, n_init=n_init, max_iter=max_iter, seed=seed)   # :76-77
        b = best_init(n, sums)
        self.set_clusters(centers[b], n[b])                                                               # :79-102
        self.set_hue_counts(dev.colors_hue())                                                             # :105
        return {"image_size": (dev.W, dev.H), "total_pixels": dev.W * dev.H, "analyzed_pixels": kept, "dominant_colors": self.dominant_colors,
                "hue_distribution": self.color_histogram}

    def recommend_colors(self, n_colors: int = 4, coverage_boost: bool = True) -> List[Tuple[str, float]]:
        """:175-242"""
        if not self.dominant_colors:
            raise ValueError("Run analyze() first")
        color_scores: Dict[str, float] = {}
        for dom_color in self.dominant_colors[: min(len(self.dominant_colors), 12)]:                      # :196
            weight = dom_color["percentage"]
            if dom_color["distance"] > 50:                                                                # :201
                weight *= 0.5
            color_scores[dom_color["closest_palette"]] = color_scores.get(dom_color["closest_palette"], 0.0) + weight
        if coverage_boost:                                                                                # :207-216
            boosted: Dict[str, float] = {}
            for color_name, score in color_scores.items():
                for similar in self.palette.get_color_group(color_name, tolerance=40):
                    boosted[similar] = boosted.get(similar, 0.0) + (score if similar == color_name else score * 0.3)
            color_scores = boosted
        sorted_colors = sorted(color_scores.items(), key=lambda x: -x[1])                                 # :219
        names = list(self.palette.colors)
        labs8 = self.palette.labs().astype(np.uint8)
        selected: List[Tuple[str, float]] = []
        selected_labs: List[np.ndarray] = []
        for color_name, score in sorted_colors:
            if len(selected) >= n_colors:
                break
            color_lab = labs8[names.index(color_name)]                                                    # :229-231
            # :233 as written: both operands are uint8, so the difference wraps modulo 256 before the norm
            too_similar = any(float(np.sqrt(((color_lab - lab).astype(np.float64) ** 2).sum())) < 30 for lab in selected_labs)
            if not too_similar:
                selected.append((color_name, score))
                selected_labs.append(color_lab)
        selected.sort(key=lambda x: -np.mean(self.palette.colors[x[0]]))                                  # :239 light -> dark
        self.recommendations = selected
        return selected

    def visualize_analysis(self, save_path: str) -> None:
        """:244-319, the four panels, on the Agg backend: nothing here has a display, so the figure is always saved"""
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        fig, axes = plt.subplots(2, 2, figsize=(12, 10))
        ax = axes[0, 0]
        colors = [d["rgb"] for d in self.dominant_colors[:8]]
        ax.bar(range(len(colors)), [d["percentage"] for d in self.dominant_colors[:8]], color=[(r / 255, g / 255, b / 255) for r, g, b in colors])
        ax.set_xlabel("Dominant Colors"); ax.set_ylabel("Percentage (%)"); ax.set_title("Dominant Colors in Image")
        ax.set_xticks(range(len(colors))); ax.set_xticklabels([f"C{i+1}" for i in range(len(colors))])
        ax = axes[0, 1]
        if self.color_histogram:
            pairs = [p for p in sorted(self.color_histogram.items(), key=lambda x: -x[1])[:8] if p[1] > 0]
            if pairs:
                ax.pie([p[1] for p in pairs], labels=[p[0] for p in pairs], autopct="%1.1f%%")
            ax.set_title("Hue Distribution")
        ax = axes[1, 0]
        y_pos = 0
        for dom_color in self.dominant_colors[:6]:
            ax.imshow(np.array(dom_color["rgb"], np.uint8).reshape(1, 1, 3), extent=[0, 1, y_pos, y_pos + 0.8])
            name = dom_color["closest_palette"]
            ax.imshow(np.array(self.palette.colors[name], np.uint8).reshape(1, 1, 3), extent=[1.2, 2.2, y_pos, y_pos + 0.8])
            ax.text(2.4, y_pos + 0.4, f"{name}\n(dist: {dom_color['distance']:.1f})", va="center", fontsize=9)
            y_pos += 1
        ax.set_xlim(-0.1, 4); ax.set_ylim(-0.5, y_pos); ax.set_aspect("auto"); ax.set_title("Original -> Palette Mapping")
        ax.set_xticks([0.5, 1.7]); ax.set_xticklabels(["Original", "Palette"]); ax.set_yticks([])
        ax = axes[1, 1]
        if self.recommendations:
            rec_names = [r[0] for r in self.recommendations]
            ax.barh(range(len(rec_names)), [r[1] for r in self.recommendations], color=[tuple(c / 255 for c in self.palette.colors[n]) for n in rec_names])
            ax.set_yticks(range(len(rec_names))); ax.set_yticklabels(rec_names)
            ax.set_xlabel("Coverage Score"); ax.set_title(f"Recommended {len(rec_names)} Colors"); ax.invert_yaxis()
        plt.suptitle("Color Analysis Results", fontsize=14, fontweight="bold")
        plt.tight_layout()
        plt.savefig(save_path, dpi=150, bbox_inches="tight")
        plt.close(fig)
        print(f"Visualization saved to {save_path}")


def recommendations_json(image: str, palette: Palette, recommendations: Sequence[Tuple[str, float]]) -> dict:
    """:394-406, the layout orip.colors.palette_from_json reads"""
    return {"image": image,
            "recommended_colors": [{"position": i, "name": name, "rgb": list(palette.colors[name]), "coverage": float(score)}
                                   for i, (name, score) in enumerate(recommendations, 1)]}
