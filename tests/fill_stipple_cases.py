"""Named inputs of orip_fill_stipple: masks of at most 96 x 128 on canvases of at most about 400 x 300, a few thousand candidates each.  A case is the dict
args() unpacks for orip.device.Device.fill_stipple and for tests/fill_stipple_double.fill_stipple alike.  PINNED holds the counts a CPU prototype of the
rule gave, which the cases are held to beside the double."""
import numpy as np

SERPENTINE = 1


def case(mask, tone, W, H, place, lattice, clear_rad=0, tone_rad=0, lo=0, hi=255, flags=SERPENTINE):
    return dict(mask=np.ascontiguousarray(mask, np.uint8), tone=None if tone is None else np.ascontiguousarray(tone, np.uint8), W=W, H=H, place=tuple(place),
                lattice=tuple(lattice), clear_rad=clear_rad, tone_rad=tone_rad, lo=lo, hi=hi, flags=flags)


def args(c):
    return c["mask"], c["tone"], c["W"], c["H"], c["place"], c["lattice"], c["clear_rad"], c["tone_rad"], c["lo"], c["hi"], c["flags"]


FLAT = {255: 0, 254: 4, 192: 64, 128: 128, 64: 192, 1: 256, 0: 256}                        # grey -> dots: periods x #{T : 64 d > 255 T}, d = 255 - grey, four periods
PINNED = {f"flat_{g}": dict(candidates=256, ink=256, near=0, light=256 - n, dots=n) for g, n in FLAT.items()}
PINNED["bleed"] = dict(candidates=400, ink=200, near=0, light=200, dots=0)
PINNED["ramp"] = dict(candidates=4134, ink=3625, near=217, light=1620, dots=1788)


def blob(h, w, seed, p=0.5):
    """a seeded random mask with connected stretches: noise smoothed by a 5 x 5 box, cut at its quantile"""
    rng = np.random.RandomState(seed)
    n = np.pad(rng.rand(h, w), 2, mode="edge")
    s = sum(n[a:a + h, b:b + w] for a in range(5) for b in range(5))
    return ((s > np.quantile(s, 1 - p)) * 255).astype(np.uint8)


def cases():
    out = {}
    full64 = np.full((64, 64), 255, np.uint8)
    for g in FLAT:                                                                        # 16 x 16 candidates: four whole Bayer periods
        out[f"flat_{g}"] = case(full64, np.full((64, 64), g), 64, 64, (1, 1, 0, 0), (4, 4, 0), 0, 2, flags=0)
    half = np.zeros((40, 40), np.uint8); half[:, 20:] = 255                               # white where set, black beside it: nothing bleeds in
    out["bleed"] = case(half, np.where(half != 0, 255, 0), 40, 40, (1, 1, 0, 0), (2, 2, 1), 0, 32)
    m = np.full((64, 96), 255, np.uint8); m[:, 0:3] = 0
    ramp = np.tile(np.linspace(255, 0, 96).astype(np.uint8), (64, 1))                      # light on the left, dark on the right
    out["ramp"] = case(m, ramp, 234, 158, (7, 3, 5, 5), (3, 3, 1), 1, 3)
    rng = np.random.RandomState(5)
    bl = blob(48, 64, 3, 0.6)
    tn = rng.randint(0, 256, (48, 64)).astype(np.uint8)
    out["rational"] = case(bl, tn, 150, 110, (7, 3, -9, -13), (5, 4, 2), 1, 2)            # floor division on negatives; candidates left of and above the image
    out["rational_off"] = case(bl, tn, 200, 140, (5, 3, 23, 17), (4, 3, 1), 0, 1)         # candidates left of, above, right of and below the image
    touch = np.full((96, 128), 255, np.uint8); touch[12:16, 20:30] = 0                    # touches all four borders: the outside counts as unset
    tt = rng.randint(0, 256, (96, 128)).astype(np.uint8)
    for cr, lat in ((0, (9, 8, 4)), (1, (9, 8, 4)), (32, (7, 6, 3))):
        out[f"border_clear{cr}"] = case(touch, tt, 128, 96, (1, 1, 0, 0), lat, cr, 1)
    cm = np.zeros((70, 90), np.uint8); cm[:30, :30] = 255; cm[:30, -30:] = 255; cm[-30:, :30] = 255; cm[-30:, -30:] = 255; cm[33:37, :] = 255
    ct = rng.randint(0, 256, (70, 90)).astype(np.uint8)
    for tr in (0, 3, 4, 32):                                                              # windows clipped at the image corners; 3 and 4 lie on either side of the path switch
        out[f"radii_tone{tr}"] = case(cm, ct, 90, 70, (1, 1, 0, 0), (6, 5, 3), 0, tr)
    out["radii_clear4"] = case(cm, ct, 90, 70, (1, 1, 0, 0), (3, 3, 1), 4, 3)             # the wave walks the clearance, the lane the tone
    out["radii_both32"] = case(touch, tt, 256, 192, (2, 1, 0, 0), (13, 11, 6), 32, 32)
    tl = np.full((48, 64), 155, np.uint8)                                                 # darkness 100
    out["lohi_below"] = case(bl, tl, 192, 144, (3, 1, 0, 0), (4, 4, 2), 1, 2, lo=100, hi=101)      # at lo: nothing
    out["lohi_at"] = case(bl, tl - 1, 192, 144, (3, 1, 0, 0), (4, 4, 2), 1, 2, lo=100, hi=101)     # at hi: every clear candidate
    out["tone_none"] = case(bl, None, 192, 144, (3, 1, 0, 0), (4, 4, 2), 1, 4)
    out["tone_zero"] = case(bl, np.zeros((48, 64)), 192, 144, (3, 1, 0, 0), (4, 4, 2), 1, 4)
    wide = blob(12, 100, 9, 0.7)
    wt = rng.randint(0, 200, (12, 100)).astype(np.uint8)
    for name, fl in (("serpentine", SERPENTINE), ("plain", 0)):                          # 150 candidates a row: the reversal crosses wave boundaries
        out[f"rows_{name}"] = case(wide, wt, 300, 36, (3, 1, 0, 0), (2, 3, 1), 0, 1, flags=fl)
    out["min_pitch"] = case(bl, tn, 128, 96, (2, 1, 0, 0), (2, 2, 1), 1, 1)
    out["empty"] = case(np.zeros((48, 64)), tn, 192, 144, (3, 1, 0, 0), (4, 4, 2), 1, 2)
    off = np.zeros((48, 64), np.uint8); off[1::2, 1::2] = 255                             # set only where no candidate's source pixel falls
    out["off_ink"] = case(off, tn, 64, 48, (1, 1, 0, 0), (2, 2, 0), 0, 2)
    out["single"] = case(full64, np.full((64, 64), 3), 3, 2, (1, 1, 0, 0), (4, 4, 2), 0, 1)      # a canvas smaller than the pitch: the origin alone
    for seed in (1, 2, 3):
        mk, tg = blob(80, 112, 20 + seed, 0.4 + 0.1 * seed), np.random.RandomState(40 + seed).randint(0, 256, (80, 112)).astype(np.uint8)
        out[f"random_{seed}"] = case(mk, tg, 300 + seed, 220 - seed, (8, 3, 2 - seed, 3), (3 + seed, 3 + seed, seed), seed - 1, 2 * seed, lo=10 * seed, hi=255 - 20 * seed,
                                     flags=seed & 1)
    return out


def launch_cap():
    """FS_BLOCKS of csrc/fill_stipple.hip: the unit's strided launches have at most this many workgroups of four waves, a wave per block of 64 candidates"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omnirevolve-image-processor_amd", "csrc", "fill_stipple.hip")).read()
    assert "const dim3 b(256), gw((unsigned)std::min<u64>((g.Z + 3) / 4, FS_BLOCKS));" in src
    assert src.count("for (u64 z = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); z < g.Z; z += (u64)gridDim.x * 4)") == 2
    assert "hipLaunchKernelGGL(k_fs_verdict, gw, b," in src and "hipLaunchKernelGGL(k_fs_emit, gw, b," in src
    return int(re.search(r"constexpr int FS_BLOCKS = (\d+);", src).group(1))


def blocks(c):
    """the blocks of 64 candidates of a case: rows x ceil(candidates of an even row / 64)"""
    return ((c["H"] - 1) // c["lattice"][1] + 1) * (((c["W"] - 1) // c["lattice"][0] + 1 + 63) // 64)


def past_the_cap():
    """rows of three blocks, 150 candidates each, and a third of a pass more of them than one launch of 4 FS_BLOCKS waves holds: every wave strides, most twice;
    clear_rad = tone_rad = 0, so closed_form answers"""
    rows = (4 * launch_cap() + 2) // 3 + launch_cap() // 2
    h, w = (2 * rows + 5) // 4 + 1, (300 + 3) // 4 + 1
    rng = np.random.RandomState(77)
    return case((rng.rand(h, w) < 0.6) * 255, rng.randint(0, 256, (h, w)), 300, 2 * rows, (4, 1, -3, -5), (2, 2, 1), 0, 0, lo=20, hi=230)


# the cases with both radii 0 are none of the above on purpose (every one runs a window): these are the small ones closed_form is shown equal to the double on
def zero_radius_cases():
    c = cases()
    return {k: dict(v, clear_rad=0, tone_rad=0) for k, v in c.items() if k in ("ramp", "rational", "rational_off", "rows_serpentine", "rows_plain", "min_pitch", "empty",
                                                                                "off_ink", "single", "tone_none", "random_1", "random_2", "random_3", "lohi_at", "flat_128")}
