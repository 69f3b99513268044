# 14_preview_stream.py -- drop-in for the reference stage of the same name, headless: plot_stream.bin -> plot_stream_preview.png (what the pen
# draws, replayed from the stream) + plot_stream_preview.json (the previewer's statistics).  The reference opens an interactive pygame window over
# shared/omnirevolve_plotter_stream_previewer.py with these parameters; here decode, replay and raster run on the GPU (orip/stream_preview.py,
# csrc/stream_preview.hip).  The interactive viewer is not provided.
import json
import sys
from pathlib import Path

import stage_io as _io  # noqa: F401  (puts the package directory on sys.path)
from orip import stream_preview as SP
from orip.config import load_config
from orip.device import Device


def main():
    cfg = load_config()
    outdir = Path(cfg.output_dir)
    stream = outdir / "plot_stream.bin"
    if not stream.exists():
        raise SystemExit(f"[preview] ERROR: stream file not found: {stream}")
    W, H, invert_y = SP.canvas_for_output(str(outdir), cfg)
    palette = tuple(SP.parse_color(s) for s in ("255,0,0", "0,255,0", "0,0,255", "0,0,0"))     # RGBK, the stage's mapping
    rw, rh = SP.render_size(1200, 900)
    print(f"[preview] canvas {W}x{H} steps, invert_y={invert_y}, render {rw}x{rh} px")
    dev = Device(0)
    try:
        rgb, st = SP.preview(dev, stream.read_bytes(), W, H, rw, rh, invert_y=bool(invert_y), clip=True, render_taps=True, background_white=True,
                             palette=palette)
    finally:
        dev.close()
    png = outdir / "plot_stream_preview.png"
    SP.save_png(rgb, str(png))
    (outdir / "plot_stream_preview.json").write_text(json.dumps(st, indent=2), encoding="utf-8")
    print(f"[preview] Image saved: {png}")
    SP.print_stats(st, file=sys.stdout)


if __name__ == "__main__":
    main()
