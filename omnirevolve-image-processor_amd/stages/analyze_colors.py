#!/usr/bin/env python3
# analyze_colors.py -- GPU counterpart of the reference's marker-recommendation tool: same command line (input, -n, -c, --palette, --no-boost, -v, -o,
# --show-all), the same report sections and the same <stem>_colors.json, which process_colors.py --mode palette --palette reads.
# Compute: liborip.so (colour table of every pixel: orip_colors_table; hue buckets: orip_colors_hue; weighted k-means: orip_colors_kmeans; Lab of the
# palette: orip_lab_of_rgb).  The palette is orip.analyze.Palette: the reference's CariocaPalette module does not exist, the built-in default is a generic
# marker set of our own.
import argparse
import json
import sys
from pathlib import Path

import stage_io as _io
from orip import analyze as AN
from orip.device import Device


def _cli(argv):
    p = argparse.ArgumentParser(description="Analyze image colors and recommend markers (GPU)")
    p.add_argument("input", help="Input image path")
    p.add_argument("-n", "--num-colors", type=int, default=4, help="Number of colors to recommend (default: 4)")
    p.add_argument("-c", "--clusters", type=int, default=8, help="Number of color clusters for analysis (default: 8)")
    p.add_argument("--palette", help="Custom palette JSON file")
    p.add_argument("--no-boost", action="store_true", help="Disable coverage boosting for similar colors")
    p.add_argument("-v", "--visualize", action="store_true", help="Save the visualization next to the JSON (there is no display)")
    p.add_argument("-o", "--output", help="Save visualization to file")
    p.add_argument("--show-all", action="store_true", help="Print all dominant colors with palette matches")
    return p.parse_args(argv)


def run(opts) -> int:
    bgr = _io.read_bgr(opts.input)
    if bgr is None:
        raise ValueError(f"Cannot load image: {opts.input}")
    dev = Device(0)
    try:
        if opts.palette:
            palette = AN.Palette.load(opts.palette, dev.lab_of_rgb)
            print(f"Loaded custom palette from {opts.palette}")
        else:
            palette = AN.Palette(None, dev.lab_of_rgb)
            print(f"Using default marker palette ({len(palette.colors)} colors)")
        dev.set_image(bgr)
        analyzer = AN.ColorAnalyzer(palette)
        results = analyzer.analyze(dev, n_clusters=opts.clusters)
        recommendations = analyzer.recommend_colors(n_colors=opts.num_colors, coverage_boost=not opts.no_boost)
        groups = {name: palette.get_color_group(name, tolerance=35) for name, _ in recommendations}
    finally:
        dev.close()

    print("\n" + "=" * 50)
    print(f"Image: {opts.input}")
    print(f"Size: {results['image_size'][0]}x{results['image_size'][1]}")
    print(f"Analyzed pixels: {results['analyzed_pixels']:,}")
    print("\n" + "=" * 50)
    print("Dominant colors:")
    shown = results["dominant_colors"] if opts.show_all else results["dominant_colors"][:8]
    for i, color in enumerate(shown, 1):
        print(f"  {i}. RGB{color['rgb']} ({color['percentage']:.1f}%)")
        print(f"     → {color['closest_palette']} (distance: {color['distance']:.1f})")
    print("\n" + "=" * 50)
    print(f"RECOMMENDED MARKERS ({opts.num_colors}):")
    print("Order: light → dark (for clean overlapping)")
    print("")
    for i, (name, score) in enumerate(recommendations, 1):
        print(f"  Position {i}: {name}")
        print(f"    RGB: {palette.colors[name]}")
        print(f"    Coverage score: {score:.1f}")
        if not opts.no_boost and len(groups[name]) > 1:
            print(f"    Also covers: {', '.join([c for c in groups[name] if c != name][:3])}")
        print()

    output_json = Path(opts.input).stem + "_colors.json"
    with open(output_json, "w") as f:
        json.dump(AN.recommendations_json(opts.input, palette, recommendations), f, indent=2)
    print(f"Recommendations saved to {output_json}")
    if opts.visualize or opts.output:
        analyzer.visualize_analysis(opts.output or (Path(opts.input).stem + "_colors.png"))
    return 0


if __name__ == "__main__":
    sys.exit(run(_cli(sys.argv[1:])))
