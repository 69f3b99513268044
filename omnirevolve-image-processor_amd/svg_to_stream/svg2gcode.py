#!/usr/bin/env python3
"""svg2gcode.py -- SVG -> G-code fitted onto a page, for the reference's svg_to_stream/svg2gcode.py: same command line (plus --tolerance-mm), same fit
(bounding box, aspect-preserving scale, margins, coordinates as %.4f).  Curves are flattened, boxed and fitted on the GPU (orip.svg, liborip.so); there is no
CPU path.  The points chosen for a curve are this project's, held to the curve within --tolerance-mm; they are not the svg_to_gcode package's.

    python svg2gcode.py drawing.svg -o drawing.gcode [--page-width-mm 210 --page-height-mm 297 --margin-mm 10] [--scale S | --scale-x SX --scale-y SY] [--tolerance-mm T]
                         [--hatch-spacing-mm S [--hatch-inset-mm I] [--hatch-direction horizontal|vertical|cross] [--no-serpentine] [--hatch-fill stated|all]
                          [--hatch-angle-deg A]]      (ours: the hatch along any angle, exact on the step grid)
                         [--pen-colors rgbk|LIST]      (ours: a T<pen> line wherever the pen changes)
The options that only change how the stream is drawn (--ring-entry, --loop-start and the other stroke passes) belong to svg2stream.py: this file is the same with them.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from orip.svg import main_gcode  # noqa: E402

if __name__ == "__main__":
    main_gcode()
