"""Inputs for the component sort keys of stage 08-B (csrc/vector08b.hip: k_comp_keys, one thread per skeleton pixel, a segmented minimum over the wave, one
atomicMin per wave and component).  A case is (id, W, H, polylines, overrides of orip_params08 fields), run under skel_merge_cases.CFG like the cases of
tests/skel_path_cases.py; tests/test_oracle_comp_key_cases.py (CPU) asserts the component sizes and key properties named here on the oracle.

Two components of ONE group cannot share a 2 x 2 block: two pixels of a block are 8-neighbours, so they belong to one component, and the block index
(y >> 1) * wb + (x >> 1) with x < 2 wb never wraps.  Equal block indices do occur between groups, where the group rank in the key's upper word
decides: `equal_block_two_groups`."""
from skel_path_cases import L, LINE300, brush_fields

B6 = dict(post_brush=6, post_minlen=2)

CASES = [
    # components of 63, 65 and 64 pixels (in the order of the input's lines), each a group of its own: one wave's worth of pixels, one less, one more
    ("sizes_63_64_65", 500, 140, [L(40, 20, 104, 84), L(200, 20, 266, 86), L(360, 20, 428, 20)], B6),
    # radius 0: an oblique line thins to 23 components of one pixel each, neighbours in the pixel list
    ("single_pixels", 200, 100, [L(40, 40, 100, 70)], dict(post_brush=1, post_minlen=2)),
    # an unfinished thinning leaves one component of 8 381 pixels: 33 blocks of the key kernel add to one word
    ("fat_8381", 400, 208, LINE300, brush_fields(128)),
    # a line that climbs one pixel from left to right: its first pixel in raster order lies in the middle, the smallest block key at its left end, 190 pixels
    # later in the list: the minimum crosses lanes and waves.  (Both lie in the component's top row of blocks, where few shapes let another component's key
    # fall between them, so the device test reads the keys themselves through ORIP_COMP_DBG rather than inferring them from the order.)
    ("late_key", 400, 250, [L(100, 101, 300, 100), L(120, 141, 280, 140)], {}),
    # two congruent groups 200 px apart: both components start in block (19, 19) of their ROI, the keys differ in the group rank alone
    ("equal_block_two_groups", 400, 500, [L(100, 100, 300, 100), L(100, 300, 299, 300)], {}),
]
CAPS = "8,8"          # ORIP_COMP_CAPS: every component above 8 pixels goes to the global class
