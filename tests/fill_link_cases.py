"""Named inputs of orip_fill_link: every case of tests/fill_cases.py at reach = 2 x and 3 x its spacing, and the cases below, each the smallest shape at
which one of the kernels of csrc/fill_link.hip can go wrong.  Masks of at most 64 x 48 on canvases of at most 300 x 300 (cap_pairs, which has to exceed a
launch cap, aside).  A case is a case of fill_cases with the key `reach` added; args() unpacks it for tests/fill_link_double.fill_link, and
fill_cases.args() for the fill in front of it."""
import numpy as np

import fill_cases as FC
from fill_cases import ACROSS, ALONG, SERPENTINE

# csrc/fill_link.hip: k_fk_elig runs FK_BLOCKS = 2048 blocks of four waves at the most, a wave a pair; with more pairs in reach than this the waves stride
ELIG_WAVES_CAP = 2048 * 4


def args(c):
    return FC.args(c) + (c["reach"],)


def link_case(reach, *a, **kw):
    return dict(FC.case(*a, **kw), reach=reach)


def comb_mask():
    """one long run on the line y = 0, ending at x = 20; ink below it; teeth on the line y = 4 that START at x = 2, 9, 17 and 23"""
    m = np.zeros((8, 40), np.uint8)
    m[0, 0:21] = 255
    m[1:4, 0:31] = 255
    for x0, x1 in ((2, 5), (9, 12), (17, 19), (23, 26)):
        m[4, x0:x1 + 1] = 255
    return m


def cases():
    out = {}
    for name, c in FC.cases().items():
        for mult in (2, 3):
            out[f"{name}@{mult}"] = dict(c, reach=mult * c["spacing"])
    tall = np.full((64, 16), 255, np.uint8)                                           # at scale 5: 80 x 320 canvas pixels
    # the even lines end at x = 39 and the odd ones start there, 70 pixels below: links of 71 pixels, so a wave takes a second block of 64
    out["long_link"] = link_case(100, tall, 40, 300, (5, 1, 0, 0), (4096, 0), 70)
    holed = tall.copy(); holed[13, 7] = 0                                             # canvas x 35 .. 39, y 65 .. 69: pixels 65 .. 69 of the link (39, 0) -> (39, 70), none of the first 64
    out["hole_in_second_block"] = link_case(100, holed, 40, 300, (5, 1, 0, 0), (4096, 0), 70)
    slit = np.zeros((13, 30), np.uint8); slit[0:6, 3:27] = 255; slit[7:13, 3:27] = 255    # lines y = 0, 4 | 8, 12: mask row 6 is empty between y = 4 and y = 8
    out["slit"] = link_case(8, slit, 30, 13, (1, 1, 0, 0), (4096, 0), 4)
    # END (20, 0); the STARTs (9, 4), (17, 4) and (23, 4) are in reach, (17, 4) and (23, 4) tie at d^2 = 25 and both links run over ink: the lower index wins
    out["comb"] = link_case(12, comb_mask(), 40, 8, (1, 1, 0, 0), (4096, 0), 4, flags=ALONG)
    full = np.full((48, 64), 1, np.uint8)
    # reach beyond the canvas diagonal: every segment of the last row along is in reach of every segment of the first row across
    out["family_boundary"] = link_case(45, full, 30, 30, (1, 1, 0, 0), (4096, 0), 4, flags=SERPENTINE | ALONG | ACROSS)
    out["chain_150"] = link_case(4, np.full((60, 8), 255, np.uint8), 40, 300, (5, 1, 0, 0), (4096, 0), 2)      # 150 lines, one chain: past seven rounds of pointer jumping
    out["negative_k_serpentine"] = link_case(10, full, 60, 50, (1, 1, 0, 0), (2896, 2896), 5)
    out["plain_far"] = link_case(300, full, 200, 20, (4, 1, 0, 0), (4096, 0), 6, flags=ALONG)      # from the right end of a line to the left end of the next
    out["reach_1"] = dict(FC.cases()["rect_hole_p0_u0"], reach=1)
    return out


def cap_pairs():
    """more pairs in reach than ELIG_WAVES_CAP: stripes three pixels wide, one apart, on 32 lines two pixels apart.  The END of a stripe's segment is in reach
    of the STARTs of its own stripe and of the next one on the line below; the link to its own stripe runs over ink, the other one crosses the gap."""
    m = np.zeros((64, 600), np.uint8)
    m[:, np.arange(600) % 4 != 3] = 255
    return link_case(6, m, 600, 64, (1, 1, 0, 0), (4096, 0), 2, flags=ALONG)
