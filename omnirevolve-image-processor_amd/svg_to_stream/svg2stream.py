#!/usr/bin/env python3
"""svg2stream.py -- SVG -> G-code -> plotter stream -> preview, for the reference's svg_to_stream/svg2stream.py: same command line (plus --tolerance-mm), same
default output names (<stem>.gcode, <stem>_stream.bin), in one process instead of three.  The geometry stays on the GPU from the control points to the
stream bytes (orip.svg, orip.gcode, liborip.so); the G-code file is written from the fitted paths on the way.  Unless --no-preview is given the stream is
decoded and drawn on the GPU into <stem>_stream_preview.png (orip.stream_preview: what the reference shows in a window).  There is no CPU path.

    python svg2stream.py drawing.svg [-o stream.bin] [--gcode-output drawing.gcode] [--steps-per-mm 40] [--scale S] [--no-reorder] [--no-preview] [--hatch-spacing-mm S [--hatch-angle-deg A] [--hatch-connect [--hatch-connect-mm M]] ...] ...
                          [--pen-colors rgbk|LIST [--pen-order 3,0,...]] [--allow-reverse]      (ours: a pen per stroke colour, drawn pen after pen)
                          [--ring-entry] [--loop-start]      (ours: the order enters a circle, a rectangle or a closed path at its nearest vertex; the G-code file is not changed)
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from orip.svg import main_stream  # noqa: E402

if __name__ == "__main__":
    main_stream()
