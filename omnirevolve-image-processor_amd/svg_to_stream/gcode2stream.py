#!/usr/bin/env python3
"""gcode2stream.py -- G-code -> plotter stream, drop-in for the reference's svg_to_stream/gcode2stream.py: same command line, same output file, byte for byte.
The conversion to steps, the nearest-neighbour order of the paths and the packing of the stream run on the GPU (orip.gcode, liborip.so); there is no CPU path.

    python gcode2stream.py drawing.gcode -o stream.bin [--steps-per-mm 40] [--invert-y 1] [--speed-scale 1.5] [--no-reorder] ...
                           [--tool-pens [--pen-order 3,0,...]] [--allow-reverse]      (ours: pens from the T words, strokes drawn backwards where that is nearer)
                           [--ring-entry] [--loop-start]      (ours: the order enters a closed stroke at its nearest vertex; the seams of the sequence are then chosen together)
                           [--arcs [--arc-tolerance-mm T]]      (ours: G2 / G3 are drawn as the arcs they state, flattened on the GPU; without it they are chords)
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from orip.gcode import main  # noqa: E402

if __name__ == "__main__":
    main()
