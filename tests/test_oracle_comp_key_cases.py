"""The cases of tests/comp_key_cases.py are what they say, shown on the oracle with the helpers of tests/test_oracle_skel_path_cases.py.  CPU only."""
import numpy as np

import comp_key_cases as K
import test_oracle_skel_path_cases as T

BY_ID = {c[0]: c for c in K.CASES}


def groups_of(name):
    _, W, H, polys, over = BY_ID[name]
    lines, taps, lines2, merged = T.run(W, H, polys, over)
    d, _ = T.prm_of(W, H, over)
    return T.analyse(lines2, d), merged


def block_keys(g, c):
    x0, y0, x1, y1 = g["roi"]; wb = (max(1, x1 - x0) + 1) >> 1
    ys, xs = np.nonzero(c["mask"])                       # raster order: the order of the device's pixel list inside a component
    return (ys >> 1) * wb + (xs >> 1)


def test_component_sizes_around_a_wave():
    groups, merged = groups_of("sizes_63_64_65")
    assert sorted(c["S"] for g in groups for c in g["comps"]) == [63, 64, 65] and len(groups) == 3 and len(merged) == 3


def test_single_pixel_components():
    groups, _ = groups_of("single_pixels")
    (g,) = groups
    assert [c["S"] for c in g["comps"]] == [1] * 23


def test_fat_component():
    groups, merged = groups_of("fat_8381")
    (g,) = groups
    assert max(c["S"] for c in g["comps"]) == 8381 >= 4097 and len(merged) >= 1


def test_smallest_key_late_in_raster_order():
    groups, merged = groups_of("late_key")
    (g,) = groups
    assert len(g["comps"]) == 2 and len(merged) == 2
    k = block_keys(g, g["comps"][0])
    assert int(np.argmin(k)) >= 128 and k.min() < k[0], "the minimum lies more than two waves behind the component's first pixel"


def test_equal_block_index_in_two_groups():
    groups, merged = groups_of("equal_block_two_groups")
    assert len(groups) == 2 and len(merged) == 2
    (a,), (b,) = groups[0]["comps"], groups[1]["comps"]
    assert block_keys(groups[0], a).min() == block_keys(groups[1], b).min()
